#include "host_logic.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

namespace relax {
namespace host {

void StateDict::add(const char* name, const float* data, int64_t n, bool strip_module) {
    if (!name) return;
    std::string k(name);
    if (strip_module && k.rfind("module.", 0) == 0) k = k.substr(7);
    t[k] = {data, n};
}

int64_t StateDict::numel(const std::string& key) const {
    auto it = t.find(key);
    return it == t.end() ? -1 : it->second.second;
}

const float* StateDict::get(const std::string& key, int64_t n, std::string& err, const char* what) const {
    char buf[512];
    auto it = t.find(key);
    if (it == t.end()) {
        snprintf(buf, sizeof(buf), "%s: missing key '%s'", what, key.c_str());
        err = buf;
        return nullptr;
    }
    if (n > 0 && it->second.second != n) {
        snprintf(buf, sizeof(buf), "%s: key '%s' has %lld elements, expected %lld", what, key.c_str(),
                 (long long)it->second.second, (long long)n);
        err = buf;
        return nullptr;
    }
    if (!it->second.first) {
        snprintf(buf, sizeof(buf), "%s: key '%s' has a NULL data pointer", what, key.c_str());
        err = buf;
        return nullptr;
    }
    return it->second.first;
}

void fold_bn(const float* gamma, const float* beta, const float* mean, const float* var, float eps, int channels, float* scale,
             float* shift) {
    for (int o = 0; o < channels; ++o) {
        scale[o] = gamma[o] / std::sqrt(var[o] + eps);
        shift[o] = beta[o] - mean[o] * scale[o];
    }
}

bool read_bn(const StateDict& sd, const std::string& prefix, int channels, float eps, float* scale, float* shift, std::string& err) {
    const float* g = sd.get(prefix + ".weight", channels, err);
    const float* b = g ? sd.get(prefix + ".bias", channels, err) : nullptr;
    const float* mu = b ? sd.get(prefix + ".running_mean", channels, err) : nullptr;
    const float* var = mu ? sd.get(prefix + ".running_var", channels, err) : nullptr;
    if (var) fold_bn(g, b, mu, var, eps, channels, scale, shift);
    return var != nullptr;
}

// A row's sum stays sequential in column order (its bits are the contract); rows are independent, so four of them advance together: one
// chain of double additions is bound by the addition's latency, and VGG-16's fc1 alone has 10^8 terms.
void conv_hoelder(const float* rows, const float* bias_or_null, int cout, int k, float* l1max, float* bmax) {
    *l1max = 0.f;
    *bmax = 0.f;
    auto row_done = [&](double l1) { *l1max = std::fmax(*l1max, (float)(l1 * (1.0 + 1e-6))); };
    int o = 0;
    for (; o + 4 <= cout; o += 4) {
        const float *r0 = rows + (size_t)o * k, *r1 = r0 + k, *r2 = r1 + k, *r3 = r2 + k;
        double a = 0.0, b = 0.0, c = 0.0, d = 0.0;
        for (int kk = 0; kk < k; ++kk) {
            a += std::fabs((double)r0[kk]);
            b += std::fabs((double)r1[kk]);
            c += std::fabs((double)r2[kk]);
            d += std::fabs((double)r3[kk]);
        }
        row_done(a); row_done(b); row_done(c); row_done(d);
    }
    for (; o < cout; ++o) {
        double l1 = 0.0;
        for (int kk = 0; kk < k; ++kk) l1 += std::fabs((double)rows[(size_t)o * k + kk]);
        row_done(l1);
    }
    for (o = 0; bias_or_null && o < cout; ++o) *bmax = std::fmax(*bmax, std::fabs(bias_or_null[o]));
}

int conv_kpad(int k, int cin_pad) { return ((k * k * cin_pad + 31) / 32) * 32; }

void pack_conv_oihw(const float* w, const float* scale, int cout, int cin, int cin_pad, int k, int kpad, float* out) {
    for (size_t i = 0, n = (size_t)cout * kpad; i < n; ++i) out[i] = 0.f;
    for (int o = 0; o < cout; ++o) {
        const float sc = scale ? scale[o] : 1.f;
        for (int c = 0; c < cin; ++c)
            for (int dy = 0; dy < k; ++dy)
                for (int dx = 0; dx < k; ++dx)
                    out[(size_t)o * kpad + (size_t)(dy * k + dx) * cin_pad + c] = w[(((size_t)o * cin + c) * k + dy) * k + dx] * sc;
    }
}

void fold_fc_bn(const float* w1, const float* b1, const float* gamma, const float* beta, const float* mean, const float* var,
                float eps, int h1, int f, int fpad, float* w1p, float* b1p) {
    for (int o = 0; o < h1; ++o) {
        const float s = gamma[o] / std::sqrt(var[o] + eps);
        for (int i = 0; i < f; ++i) w1p[(size_t)o * fpad + i] = w1[(size_t)o * f + i] * s;
        for (int i = f; i < fpad; ++i) w1p[(size_t)o * fpad + i] = 0.f;
        b1p[o] = (b1[o] - mean[o]) * s + beta[o];
    }
}

TailSplit choose_tail_split(int ntiles, int slots, int nk, int min_steps, bool can_split) {
    TailSplit r{ntiles, 1};
    if (!can_split || ntiles <= 0 || slots <= 0 || min_steps <= 0) return r;
    const int rem = ntiles % slots;
    if (rem == 0) return r;
    int best_s = 1;
    double best = 1.0;
    const int smax = nk / min_steps < 16 ? nk / min_steps : 16;
    for (int S = 2; S <= smax; ++S) {
        const double t = (double)((rem * S + slots - 1) / slots) / S + 0.04 * S;
        if (t < best - 0.05) {
            best = t;
            best_s = S;
        }
    }
    if (best_s >= 2) {
        r.full_tiles = ntiles - rem;
        r.nsplit = best_s;
    }
    return r;
}

float h2_scale_for_bound(double amax) {
    if (!(amax > 0.0) || !(amax < 3.0e38)) return 1.f;
    int e;
    (void)std::frexp(amax, &e);   // amax in [2^(e-1), 2^e)
    int sh = 15 - e;
    sh = sh > 120 ? 120 : (sh < -120 ? -120 : sh);
    return std::ldexp(1.f, sh);
}

void h2_weight_row_scales(const float* W, int rows, int K, float* scale) {
    for (int n = 0; n < rows; ++n) {
        float m = 0.f;
        const float* r = W + (size_t)n * K;
        for (int k = 0; k < K; ++k) {
            const float a = std::fabs(r[k]);
            if (a > m) m = a;     // (a NaN never wins the comparison: such a row keeps the scale of its finite values)
        }
        scale[n] = h2_scale_for_bound((double)m);
    }
}

double layernorm_out_bound(const float* gamma, const float* beta, int dim) {
    const double zmax = std::sqrt((double)(dim > 1 ? dim - 1 : 1));
    double m = 0.0;
    for (int i = 0; i < dim; ++i) {
        const double v = std::fabs((double)gamma[i]) * zmax + std::fabs((double)beta[i]);
        if (v > m) m = v;
    }
    return m;
}

double linear_of_layernorm_bound(const float* W, const float* b, const float* gamma, const float* beta, int dim, int n0, int n1) {
    const double zn = std::sqrt((double)dim);
    double m = 0.0;
    for (int n = n0; n < n1; ++n) {
        const float* r = W + (size_t)n * dim;
        double q = 0.0, c = b ? (double)b[n] : 0.0;
        for (int i = 0; i < dim; ++i) {
            const double gw = (double)gamma[i] * (double)r[i];
            q += gw * gw;
            c += (double)beta[i] * (double)r[i];
        }
        const double v = zn * std::sqrt(q) + std::fabs(c);
        if (v > m) m = v;
    }
    return m;
}

}  // namespace host
}  // namespace relax

namespace relax {
namespace host {

const int kVggFeatureIndex[kVggConvs] = {0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28};
const int kVggConvCout[kVggConvs] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
const int kVggConvCin[kVggConvs] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};

bool vgg16_check_keys(const StateDict& sd, std::string& err) {
    const char* what = "vgg16 state dict";
    for (int i = 0; i < kVggConvs; ++i) {
        const std::string p = "features." + std::to_string(kVggFeatureIndex[i]);
        if (!sd.get(p + ".weight", (int64_t)kVggConvCout[i] * kVggConvCin[i] * 9, err, what)) return false;
        if (!sd.get(p + ".bias", kVggConvCout[i], err, what)) return false;
    }
    if (!sd.get("classifier.0.weight", (int64_t)4096 * 512 * 49, err, what)) return false;
    if (!sd.get("classifier.0.bias", 4096, err, what)) return false;
    if (!sd.get("classifier.3.weight", (int64_t)4096 * 4096, err, what)) return false;
    if (!sd.get("classifier.3.bias", 4096, err, what)) return false;
    return true;
}

void vgg16_fc1_to_nhwc(const float* w, int rows, int C, int HW, float* out) {
    const size_t K = (size_t)C * HW;
    for (int r = 0; r < rows; ++r) {
        const float* src = w + (size_t)r * K;
        float* dst = out + (size_t)r * K;
        for (int c = 0; c < C; ++c)
            for (int p = 0; p < HW; ++p) dst[(size_t)p * C + c] = src[(size_t)c * HW + p];
    }
}

// ---- VGG-16 schedule ---------------------------------------------------------------------------------------------------------------------
const int kVggConvSide[kVggConvs] = {224, 224, 112, 112, 56, 56, 56, 28, 28, 28, 14, 14, 14};
const int kVggPoolAfter[kVggConvs] = {0, 1, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1};

VggArena vgg_arena() {
    const int64_t map = (int64_t)224 * 224 * 64;   // the largest activation (conv1_x output) as fp32
    const int64_t planes = map * 3 / 2;            // ... as split planes (6 B per value; fp16 planes and fp32 rows take 4)
    const int64_t groups = map / 16;               // group sums of the fused mean (largest: 16-row groups at 224^2 x 64 = 4-row groups at 56^2 x 256)
    const int64_t fc = 4096;
    VggArena a{};
    a.a32 = 0;
    a.planes0 = a.a32 + map;
    a.planes1 = a.planes0 + planes;
    a.groups = a.planes1 + planes;
    a.fc1 = a.groups + groups;
    a.fc2 = a.fc1 + fc;
    a.slots = a.fc2 + fc;
    a.floats = a.slots + 3 * kVggSlots;
    return a;
}

bool vgg_plan(const VggOptions& o, const VggRequest& rq, int max_slots, VggPlan* plan, std::string& err) {
    const bool h2 = o.precision == 3, x6 = o.precision >= 2;
    VggPlan p{};
    p.arena = vgg_arena();
    p.classifier = rq.want_pool || (rq.taps >> 13 & 3u) != 0;
    p.n_rows = p.classifier ? kVggSteps : kVggSteps - 2;
    int next_slot = 0, rows = 0;
    int cur = kVggBufPlanes0, oth = kVggBufPlanes1;   // the next contraction's input (planes of the arithmetic, or fp32 rows) and the other plane buffer
    int s_in = -1, s_max = -1;                        // f16x2: the slot with the current tensor's scale, and the one with its measured maximum
    auto step = [&](int route, int layer, int side, int cin, int cout) -> VggLayerPlan& {
        VggLayerPlan& q = p.row[rows++];
        q.route = route; q.layer = layer; q.side = side; q.cin = cin; q.cout = cout;
        q.in = cur; q.out32 = kVggBufNone; q.out_planes = kVggBufNone;
        q.want_export = !vgg_is_pool(route) && (rq.taps >> layer & 1u);
        q.no_split = route == kVggConvH3 || route == kVggConvX6H2 || route == kVggConvX6;   // the bits do not depend on which outputs are requested
        q.s_in = vgg_is_pool(route) ? -1 : s_in;   // (a pool reads the fp32 map)
        q.s_in_max = s_max; q.s_out = h2 ? next_slot++ : -1;
        return q;
    };
    // the one ladder: gemm_h3 takes Cout % 256 == 0, the four-wave f16x2 tiles of gemm_x6 the rest
    auto contraction = [&](int cout) { return h2 ? (cout % 256 == 0 ? kVggConvH3 : kVggConvX6H2) : x6 ? kVggConvX6 : kVggConvF32; };
    for (int i = 0; i < kVggConvs; ++i) {
        const int side = kVggConvSide[i], hw = side * side, cout = kVggConvCout[i];
        const bool pool_next = kVggPoolAfter[i] != 0;
        VggLayerPlan& q = step(i == 0 ? kVggConv11 : contraction(cout), i, side, kVggConvCin[i], cout);
        q.want_mean = rq.want_layer_stack != 0;
        q.measure_max = h2;
        if (i == 0) {   // conv1_1 writes where the next convolution reads (its own input is the fragments); its scale is a constant of the weights
            q.in = kVggBufNone; q.s_in_max = -1;
            q.out32 = x6 ? (q.want_export ? kVggBufA32 : kVggBufNone) : cur;
            q.out_planes = x6 ? cur : kVggBufNone;
            q.gap_group = q.want_mean ? 16 : 0;
        } else {
            // under planes the fp32 copy exists iff a pool follows or the tap is exported; fp32 rows go to the other plane buffer
            q.out32 = x6 ? ((pool_next || q.want_export) ? kVggBufA32 : kVggBufNone) : oth;
            q.out_planes = (x6 && !pool_next) ? oth : kVggBufNone;
            if (x6 && q.want_mean) q.gap_group = q.route == kVggConvH3 ? 4 : hw % 16 == 0 ? 16 : 4;
        }
        s_in = s_max = q.s_out;
        if (!pool_next) {
            if (i > 0) std::swap(cur, oth);
            continue;
        }
        // the pool reads the fp32 map and writes into the buffer its producer's input came from (consumed by now): no swap.  f16x2: a new scale slot
        // from the measured maximum of the map, which bounds the pool's outputs too - the maximum slot stays the producer's
        const int src = q.out32;
        VggLayerPlan& m = step(h2 ? kVggPoolH2 : x6 ? kVggPoolSp3 : kVggPoolF32, i, side, cout, cout);
        m.in = src;
        (x6 ? m.out_planes : m.out32) = cur;
        s_in = m.s_out;
    }
    // classifier: pool5 (NHWC flatten) -> fc1 + ReLU -> fc2 + ReLU, planned whether or not it runs (n_rows ends in front of it)
    for (int i = 0; i < 2; ++i) {
        const bool last = i == 1;
        VggLayerPlan& q = step(contraction(4096), 13 + i, 1, i == 0 ? 512 * 49 : 4096, 4096);
        if (last && !x6) q.in = kVggBufFc1;
        const bool need32 = last || q.want_export || !x6;
        q.out32 = need32 ? (last ? kVggBufFc2 : kVggBufFc1) : kVggBufNone;
        q.out_planes = (x6 && !last) ? oth : kVggBufNone;
        q.measure_max = h2 && q.out_planes != kVggBufNone;
        s_in = s_max = q.s_out;
        if (q.out_planes != kVggBufNone) std::swap(cur, oth);
    }
    p.n_slots = next_slot;
    if (next_slot > max_slots) {
        err = "vgg16: " + std::to_string(next_slot) + " per-image scale slots used, " + std::to_string(max_slots) + " reserved";
        return false;
    }
    *plan = p;
    return true;
}

// ---- ResNet-50 schedule ------------------------------------------------------------------------------------------------------------------
const RnBlockGeom* rn_geometry() {
    struct Table { RnBlockGeom g[kRnBlocks]; };
    static const Table t = [] {
        Table r{};
        const int stage_blocks[4] = {3, 4, 6, 3}, stage_width[4] = {64, 128, 256, 512};
        const int stage_taps[4] = {3, 4, 4, 3};  // layer3 blocks 4, 5 are not tapped
        int cin = 64, tap = 1, b = 0;            // (tap 0 is the stem's raw conv1 output)
        for (int st = 0; st < 4; ++st)
            for (int i = 0; i < stage_blocks[st]; ++i, ++b) {
                const int w = stage_width[st];
                r.g[b] = {b, st + 1, i, cin, w, w * 4, (i == 0 && st > 0) ? 2 : 1, i == 0, i < stage_taps[st] ? tap++ : -1};
                cin = w * 4;
            }
        return r;
    }();
    return t.g;
}

bool rn_canvas_geometry(int Hc, int Wc, RnCanvasGeometry* g, std::string& err) { return rn_canvas_geometry(Hc, Wc, 0, g, err); }

bool rn_canvas_geometry(int Hc, int Wc, int flags, RnCanvasGeometry* g, std::string& err) {
    const std::string canvas = " (canvas " + std::to_string(Hc) + " x " + std::to_string(Wc) + ")";
    if (flags & ~kRnCanvasAny) {
        err = "resnet50: canvas flags " + std::to_string(flags) + " have unknown bits " + std::to_string(flags & ~kRnCanvasAny) +
              " (RELAX_RN_CANVAS_ANY = " + std::to_string(kRnCanvasAny) + " is the only flag)" + canvas;
        return false;
    }
    for (int axis = 0; axis < 2; ++axis) {
        const int v = axis == 0 ? Hc : Wc;
        const bool in_range = v >= kRnCanvasMin && v <= kRnCanvasMax;
        if (in_range && ((flags & kRnCanvasAny) || v % kRnCanvasStep == 0)) continue;
        const std::string what = std::string("resnet50: canvas ") + (axis == 0 ? "height " : "width ") + std::to_string(v);
        const std::string range = "[" + std::to_string(kRnCanvasMin) + ", " + std::to_string(kRnCanvasMax) + "]";
        err = (flags & kRnCanvasAny) ? what + " is not in " + range + canvas : what + " is not a multiple of " + std::to_string(kRnCanvasStep) + " in " + range + canvas;
        return false;
    }
    RnCanvasGeometry r{};
    const RnBlockGeom* blocks = rn_geometry();
    // conv1 7x7 / 2 pad 3, then the 3x3 / 2 pad 1 max-pool, then a 3x3 / stride pad 1 convolution per block: floor((n + 2 p - k) / s) + 1
    int H = (Hc + 2 * 3 - 7) / 2 + 1, W = (Wc + 2 * 3 - 7) / 2 + 1;
    r.tap_hw[0][0] = H; r.tap_hw[0][1] = W;
    static const int tap_c[kRnTaps] = {64, 256, 256, 256, 512, 512, 512, 512, 1024, 1024, 1024, 1024, 2048, 2048, 2048};
    H = (H + 2 - 3) / 2 + 1; W = (W + 2 - 3) / 2 + 1;
    const int64_t hw1 = (int64_t)H * W;      // layer1's maps
    r.block_max = ((hw1 * (64 / 4) + 255) / 256 + 63) / 64 * 64;
    for (int b = 0; b < kRnBlocks; ++b) {
        H = (H + 2 - 3) / blocks[b].stride + 1; W = (W + 2 - 3) / blocks[b].stride + 1;
        if (blocks[b].tap >= 0) { r.tap_hw[blocks[b].tap][0] = H; r.tap_hw[blocks[b].tap][1] = W; }
    }
    r.x0 = (int64_t)Hc * Wc * 4;
    r.big = (int64_t)r.tap_hw[0][0] * r.tap_hw[0][1] * 64;
    if (hw1 * 256 > r.big) r.big = hw1 * 256;   // (odd stem maps: the max-pool rounds up, layer1's 256-channel output is the larger tensor)
    r.t1 = hw1 * 128;
    r.t2 = hw1 * 64;
    r.gap_ws = 16 * 2048;
    for (int t = 0; t < kRnTaps; ++t) {
        const int64_t hw = (int64_t)r.tap_hw[t][0] * r.tap_hw[t][1];
        if (hw % 4 != 0) continue;                                  // (no fused mean on such a map: rn_maps_fused_mean)
        const int64_t groups = hw / (hw % 16 == 0 ? 16 : 4) * tap_c[t];
        if (groups > r.gap_ws) r.gap_ws = groups;
    }
    r.floats_f32 = r.x0 + 3 * r.big + r.t1 + r.t2 + r.gap_ws + kRnAvgFloats;
    // bf16x6 path: block inputs / outputs exist twice (fp32 for the residual add and the taps, split planes = 1.5 floats per
    // value for the next convolutions), the intermediates of a block only as split planes
    r.floats_x6 = r.x0 + 3 * r.big + 2 * (r.big * 3 / 2) + (r.t1 + r.t2) * 3 / 2 + r.gap_ws + kRnAvgFloats + 3 * kRnImgSlots + r.block_max;
    *g = r;
    return true;
}

bool rn_plan(const RnOptions& o, const RnRequest& rq, int max_slots, RnPlan* plan, std::string& err) {
    return rn_plan(o, rq, RnCanvas{}, max_slots, plan, err);
}

bool rn_plan(const RnOptions& o, const RnRequest& rq, const RnCanvas& cv, int max_slots, RnPlan* plan, std::string& err) {
    const RnBlockGeom* g = rn_geometry();
    RnCanvasGeometry geo;
    if (!rn_canvas_geometry(cv.Hc, cv.Wc, cv.flags, &geo, err)) return false;
    RnStemPlan stem;
    if (!rn_stem_plan(cv, &stem, err)) return false;
    const int H1 = geo.tap_hw[1][0], W1 = geo.tap_hw[1][1];   // layer1's maps: the max-pool's output
    RnPlan p{};
    // f16x2 for layer3 / layer4 ("gemm_precision" 3 with "rn_h2"): per-image tables {maximum, scale, 1 / scale}, one slot per tensor
    const bool use_h2 = o.precision == 3 && o.rn_h2;
    // "rn_h2_early": the 3x3 convolutions of layer1 / layer2 on f16x2 as well (gemm_x6.hip, H2 form).  Their input (conv1's output)
    // is written as fp16 planes with the image's Hoelder scale  l1max(conv1) max|block input| + max|bias|; the block input's maximum
    // is measured by its producer: the max-pool (block maxima, reduced per image) or the previous block's conv3 epilogue.
    // (the any-map max-pool posts per-image maxima on every map)
    bool use_early = use_h2 && o.rn_h2_early && (stem.pool_form == kRnPoolAny || rn_maps_pool_maxima(H1, W1, g[0].cin));
    for (int b = 0; b < kRnFirstH2Block && use_early; ++b) use_early = rn_early_h2(g[b].width, g[b].width);
    // "rn_fuse": layer1[0] back to back too, with the downsample convolution folded into its conv3 - the block input then travels as fp32 rows
    // (4 B per value instead of 6: conv1 splits them in its K loop, the fused launch reads each pixel's row as conv3's second source)
    const bool fuse0 = use_early && o.rn_fuse && o.fp32_rows && rn_can_b2b_x2(g[0]) && rn_maps_b2b(H1, W1);
    // layer2[0] (stride 2, 256 -> 512 downsample: too many channels for a second source in registers): the downsample convolution as a
    // launch of its own (f16x2, on the compact fp16 planes of the input's stride-2 sample) whose fp32 output is the residual of the
    // block's back-to-back launch (3x3 with the stride -> conv3) - instead of the 3x3 + the two-source bf16x6 conv3
    auto down_launch = [&](const RnBlockGeom& k) {
        return use_early && o.rn_fuse && o.rn_c1_h2 && o.fp32_rows && rn_can_down_launch(k) && rn_can_b2b(k) && rn_can_c1_h2(k);
    };
    int next_slot = 0;
    p.conv1_h2 = use_h2 && o.rn_h2_early;
    p.pool_f32 = fuse0;
    p.s_stem = use_early ? next_slot++ : -1;
    // A block output exists as split planes (next convolutions, next residual: hi + mid + lo is the fp32 value, exactly) and as
    // fp32 only where something needs it, and only for the images that need it: the tap export, the spatial mean of the 7x7
    // taps of the layer-stack images (49 rows per image do not divide into the 16- or 4-row groups of the mean fused into
    // the epilogue), the last block's map of the pool images.
    // The block outputs inside layer1 and layer2 (56x56x256 and 28x28x512: the widest tensors, their consumers HBM-bound) travel
    // as plain fp32 instead, 4 bytes per value where the planes take 6: the next block's conv1 (64 / 128 output columns, one
    // column tile, so every value is split exactly once, as the producer's epilogue would have) splits them inside its K loop
    // and its conv3 adds them as an fp32 residual - the same values bit for bit.  A layer's last block writes planes: the next
    // layer's first conv3 reads them as its second activation source.
    int in_form = fuse0 ? kRnF32 : kRnSp3, in_sample = kRnNoSample, s_x = -1, s_xin = p.s_stem, s_dr = -1, H = H1, W = W1;
    for (int b = 0; b < kRnBlocks; ++b) {
        const RnBlockGeom& k = g[b];
        RnBlockPlan& q = p.blk[b];
        const int Ho = (H + 2 - 3) / k.stride + 1, Wo = (W + 2 - 3) / k.stride + 1, HWo = Ho * Wo;   // (the 3x3, pad 1)
        const bool is_last = b + 1 == kRnBlocks, tapped = k.tap >= 0;
        const bool pool_needs32 = is_last && rq.want_pool && !rn_pool_from_stack(rq);
        q.want_mean = tapped && rq.n_ls > 0;
        q.want_export = tapped && ((rq.taps >> k.tap) & 1u);
        q.in_form = in_form; q.in_sample = in_sample;
        q.s_in_max = s_xin; q.s_in = s_x; q.s_dr_in = s_dr;
        q.s_c1 = q.s_t1 = q.s_t1m = q.s_t2 = q.s_out = q.s_dr_out = -1;
        bool out_f32 = false;
        if (use_h2 && !rn_early(k)) {
            // Every tensor that feeds a convolution travels as two fp16 planes with one scale per image; the scale of a tensor is fixed
            // BEFORE it is written, from Hoelder's bound on its producer (measured maxima of the producer's inputs, l1max / bmax of its
            // weights).  fp32 copies as above; the residual of a block without a downsample branch is read from the block input's PLANES.
            q.form = kRnFormH2;
            q.s_t1 = next_slot++; q.s_t2 = next_slot++; q.s_out = next_slot++;
            q.fuse_mean = q.want_mean && rn_maps_fused_mean(Ho, Wo) && HWo % 16 != 0;   // 14x14 maps: 4-row groups (gemm_h3's fused mean)
            q.no_split = tapped && rn_maps_fused_mean(Ho, Wo) && HWo % 16 != 0;
            q.out_form = is_last ? kRnNone : kRnH2;
        } else {
            const bool cur_f32 = in_form == kRnF32;
            // "rn_fuse": conv2 and conv3 back to back in one launch - the 3x3's tile never leaves the CU; conv3 on f16x2 with one scale per pixel row
            const bool fuse_x2 = b == 0 && fuse0;
            const bool fuse_dr = b > 0 && cur_f32 && down_launch(k) && rn_maps_b2b(Ho, Wo) && in_sample == kRnSampleH2;
            const bool fuse = fuse_x2 || fuse_dr || (use_early && o.rn_fuse && !k.has_down && rn_can_b2b(k) && cur_f32 && k.stride == 1 && rn_maps_b2b(Ho, Wo));
            // a layer's last block in front of a downsample block: its output travelled as three bf16 planes (6 B per value: the next block's conv1 and
            // the second source of its conv3 read planes).  Back to back it leaves as fp32 rows like the others (conv1 splits in its K loop) PLUS the
            // planes of the stride-2 sample only - all the downsample branch reads -, compacted: 4 + 1.5 bytes per value instead of 6, and conv1 reads 4
            // (fp16 planes with a per-image scale where the next block runs its downsample convolution as a launch of its own)
            const bool next_down = !is_last && g[b + 1].has_down;
            // (the sample is of even maps, and the next block runs back to back behind its downsample launch only on maps that form takes)
            const bool next_dr = next_down && fuse && down_launch(g[b + 1]) && rn_maps_sample2(Ho, Wo) && rn_maps_b2b(Ho / 2, Wo / 2);
            const bool compact = fuse && next_down && !next_dr && rn_early(g[b + 1]) && o.fp32_rows && k.cout <= 512 && rn_maps_sample2(Ho, Wo) && g[b + 1].stride == 2;
            out_f32 = o.fp32_rows && k.cout <= 512 && !is_last && (!next_down || compact || next_dr);
            q.handover = use_h2 && b + 1 == kRnFirstH2Block;
            q.pre_handover = use_h2 && b + 2 == kRnFirstH2Block;
            q.form = fuse_x2 ? kRnFormB2BX2 : fuse_dr ? kRnFormB2BDown : fuse ? kRnFormB2B : use_early ? kRnFormEarly : kRnFormX6;
            if ((q.handover || next_dr) && fuse) q.s_t1m = next_slot++;
            if (q.handover) { q.s_t2 = next_slot++; q.s_out = next_slot++; }
            if (use_early) q.s_t1 = next_slot++;
            // the maximum of this block's output: the next block's conv1 scale (early), the residual term of the hand-over block
            if (!q.handover && (use_early || q.pre_handover)) q.s_out = next_slot++;
            q.c1_h2 = use_early && cur_f32 && o.rn_c1_h2 && rn_can_c1_h2(k);
            if (q.c1_h2) q.s_c1 = next_slot++;
            if (next_dr) q.s_dr_out = next_slot++;
            q.fuse_mean = q.want_mean && rn_maps_fused_mean(Ho, Wo);
            q.no_split = !fuse && tapped && rn_maps_fused_mean(Ho, Wo);
            q.out_form = q.handover ? kRnH2 : out_f32 ? kRnF32 : kRnSp3;
            q.out_sample = compact ? kRnSampleSp3 : next_dr ? kRnSampleH2 : kRnNoSample;
        }
        // (a launch that fuses the mean when the layer stack is asked for runs unsplit either way - no_split does not look at the request: the
        // pool vector's bits do not depend on whether the layer stack is requested)
        q.need32 = out_f32 || q.want_export || (q.want_mean && !q.fuse_mean) || pool_needs32;
        // fp32 rows: every image for the next block, an export or the pool images behind the layer-stack ones, else the layer-stack images only
        q.rows32 = ((out_f32 || q.want_export || pool_needs32) ? rq.N : rq.n_ls) * HWo;
        in_form = q.out_form; in_sample = q.out_sample;
        s_x = q.out_form == kRnH2 ? q.s_out : -1;
        s_xin = q.s_out; s_dr = q.s_dr_out;
        H = Ho; W = Wo;
    }
    p.n_slots = next_slot;
    if (next_slot > max_slots) {
        err = "resnet50: " + std::to_string(next_slot) + " per-image scale slots used, " + std::to_string(max_slots) + " reserved";
        return false;
    }
    *plan = p;
    return true;
}

bool rn_stem_plan(const RnCanvas& cv, RnStemPlan* plan, std::string& err) {
    RnCanvasGeometry geo;
    if (!rn_canvas_geometry(cv.Hc, cv.Wc, cv.flags, &geo, err)) return false;
    RnStemPlan p{};
    if (rn_canvas_default_rule(cv.Hc, cv.Wc) && !((cv.flags & kRnCanvasAny) && cv.force_any)) {
        p.stem_form = cv.Hc == kRnCanvasDefault && cv.Wc == kRnCanvasDefault ? kRnStem224 : kRnStemTiles;
        p.pool_form = kRnPoolEven;
        p.stem_fused_mean = 1;
    } else {
        p.stem_form = kRnStemAny;
        p.pool_form = kRnPoolAny;
        p.stem_fused_mean = rn_maps_stem_fused_mean(geo.tap_hw[0][0], geo.tap_hw[0][1]);
    }
    *plan = p;
    return true;
}

// ---- ViT geometry, arena sizes, streaming-attention plan -------------------------------------------------------------------------------
bool vit_geometry(int patch, VitGeometry* g, std::string& err) {
    if (patch != 8 && patch != 16) {
        err = "vit: patch_size " + std::to_string(patch) + " is not built (8 or 16 at 224x224)";
        return false;
    }
    const int side = 224 / patch;
    *g = VitGeometry{patch, side, side * side, side * side + 1, 3 * patch * patch};
    return true;
}

bool vit_canvas_geometry(int patch, int Hc, int Wc, VitCanvasGeometry* g, std::string& err) {
    VitGeometry base;
    if (!vit_geometry(patch, &base, err)) return false;
    if (Hc < patch || Wc < patch) {
        const bool h_bad = Hc < patch;
        err = std::string("vit: canvas ") + (h_bad ? "height " : "width ") + std::to_string(h_bad ? Hc : Wc) + " is below the patch size " +
              std::to_string(patch) + " (canvas " + std::to_string(Hc) + " x " + std::to_string(Wc) + ")";
        return false;
    }
    const int64_t gh = Hc / patch, gw = Wc / patch, npatch = gh * gw;
    if (npatch > kVitMaxPatches) {
        err = "vit: canvas " + std::to_string(Hc) + " x " + std::to_string(Wc) + " has " + std::to_string(gh) + " x " + std::to_string(gw) + " = " +
              std::to_string(npatch) + " patches at patch size " + std::to_string(patch) + ", the limit is " + std::to_string(kVitMaxPatches) +
              " patches (" + std::to_string(kVitMaxPatches + 1) + " tokens)";
        return false;
    }
    *g = VitCanvasGeometry{(int)gh, (int)gw, (int)npatch, (int)npatch + 1, gh == base.side && gw == base.side};
    return true;
}

// What is specified: an fp32 coordinate from a double-derived scale, fp32 cubic weights.  Which of those fp32 operations are fused is not
// specified by torch: it is what its compiler contracted.  The roundings below (fmaf for the coordinate scale * (dst + 0.5) - 0.5 and the first
// Horner steps of the two cubics, a separately rounded product elsewhere) are those of torch 2.10's x86-64 CPU build, written out so that the
// taps do not depend on THIS file's compiler flags; with them the weights equal that build's bit for bit on every tap inside the table
// (tests/test_vit_canvas_cpu.py asserts it, and says what to do when another torch build contracts differently: the difference is then one
// or two ulp of a weight, far inside the gates; an unfused coordinate alone moves a weight by up to 1.2e-6 and costs the 28-wide grids their
// margin).
static inline float mul_then_add(float a, float b, float c) {
    volatile float p = a * b;   // (volatile: rounded to fp32 here, whatever the compiler may contract)
    return p + c;
}
void pos_interp_taps(int side, int g, int32_t* idx, float* w) {
    const float A = -0.75f;
    const float scale = (float)(1.0 / (((double)g + 0.1) / (double)side));
    auto conv1 = [&](float x) {   // ((A + 2) x - (A + 3)) x x + 1,  |x| <= 1
        volatile float q = std::fmaf(A + 2.f, x, -(A + 3.f)) * x;
        return mul_then_add(q, x, 1.f);
    };
    auto conv2 = [&](float x) {   // ((A x - 5 A) x + 8 A) x - 4 A,  1 <= |x| <= 2
        return mul_then_add(std::fmaf(std::fmaf(A, x, -5.f * A), x, 8.f * A), x, -4.f * A);
    };
    for (int i = 0; i < g; ++i) {
        const float real = std::fmaf(scale, (float)i + 0.5f, -0.5f);
        const float fl = std::floor(real);
        const float t = std::fmin(std::fmax(real - fl, 0.f), 1.f);   // (real - floor(real) is exact in fp32)
        const int i0 = (int)fl;
        const float x2 = 1.f - t;
        w[4 * i + 0] = conv2(t + 1.f);
        w[4 * i + 1] = conv1(t);
        w[4 * i + 2] = conv1(x2);
        w[4 * i + 3] = conv2(x2 + 1.f);
        for (int k = 0; k < 4; ++k) {
            const int j = i0 - 1 + k;
            idx[4 * i + k] = j < 0 ? 0 : (j > side - 1 ? side - 1 : j);
        }
    }
}

VitArena vit_arena(bool planes, int dim, int ntok, int npatch, int patch_k) {
    const int64_t td = (int64_t)ntok * dim, pk = (int64_t)npatch * patch_k;
    VitArena a{};
    a.embedded = planes ? pk * 3 / 2 : pk;                           // behind the patches (sp3: 3/2 floats per value)
    a.residual = a.embedded + (int64_t)npatch * dim;                 // behind the patch-embed output
    a.operand = a.residual + td;                                     // LayerNorm / attention output: what the next GEMM reads
    a.qkv = a.operand + (planes ? td * 3 / 2 : td);
    a.final = planes ? a.qkv + td * 3 : a.operand;                   // the final LayerNorm's fp32 rows
    a.hidden = planes ? a.final + td : a.qkv + td * 3;               // GELU(fc1)
    a.floats = a.hidden + (planes ? td * 4 * 3 / 2 : td * 4);
    return a;
}

VitPlan vit_plan(const VitOptions& o, const VitModel& m, const VitRequest& rq) {
    VitPlan p{};
    p.arith = o.precision == 3 && m.dim % 256 == 0 ? kVitH2 : o.precision >= 2 ? kVitX6 : kVitF32;
    p.patch_embed = p.arith == kVitH2 && m.patch == 8 ? kVitX6 : p.arith;
    const bool single_tile = rq.ntok == 197;
    p.qkv_planes = p.arith == kVitH2 && o.att_h2 && (single_tile || o.att_h2_stream);
    // (f16x2 without qkv planes: attention keeps its bf16x6 arithmetic inside and writes fp16 planes)
    p.attention = p.arith == kVitF32 ? (single_tile ? kVitAttention : kVitAttentionStreamF32)
                  : p.qkv_planes     ? (single_tile ? kVitAttentionH2 : kVitAttentionStreamH2)
                                     : (single_tile ? kVitAttentionX6 : kVitAttentionStreamX6);
    p.attention_only = rq.want_cls_attention && !rq.want_tokens && !rq.want_pooled;
    p.final_norm = rq.n_last == 0 && !p.attention_only;
    p.arena = vit_arena(p.arith != kVitF32, m.dim, rq.ntok, rq.npatch, m.patch_k);
    return p;
}

bool att_stream_plan(int Nimg, int heads, int ntok, int arith, AttStreamPlan* plan, std::string& err) {
    if (Nimg < 1 || heads < 1 || ntok < 1 || (arith != kAttStreamF32 && arith != kAttStreamX6)) {
        err = "attention_stream: Nimg=" + std::to_string(Nimg) + " heads=" + std::to_string(heads) + " ntok=" + std::to_string(ntok);
        return false;
    }
    if (((int64_t)ntok + kAttStreamKeyTile) * heads * 64 * 3 * 4 > (int64_t)INT32_MAX) {   // (the last tile's padding rows are addressed too)
        err = "attention_stream: the qkv rows of one image (" + std::to_string(ntok) + " tokens x " + std::to_string(heads) + " heads) pass 2^31 bytes";
        return false;
    }
    AttStreamPlan p;
    p.qblock = kAttStreamQBlock;
    p.qblocks = (ntok + p.qblock - 1) / p.qblock;
    p.key_tiles = (ntok + kAttStreamKeyTile - 1) / kAttStreamKeyTile;
    p.lds_bytes = arith == kAttStreamF32 ? kAttStreamLdsF32 : kAttStreamLdsX6;
    const int64_t items = (int64_t)Nimg * heads * p.qblocks;
    if (items > (int64_t)INT32_MAX) {
        err = "attention_stream: " + std::to_string(items) + " work items";
        return false;
    }
    p.items = (int)items;
    *plan = p;
    return true;
}

bool att_stream_h2_plan(int Nimg, int heads, int ntok, AttStreamH2Plan* plan, std::string& err) {
    if (Nimg < 1 || heads < 1 || ntok < 1) {
        err = "attention_stream_h2: Nimg=" + std::to_string(Nimg) + " heads=" + std::to_string(heads) + " ntok=" + std::to_string(ntok);
        return false;
    }
    if (((int64_t)ntok + kAttStreamH2KeyTile) * heads * 64 * 3 * 4 > (int64_t)INT32_MAX) {   // (the last tile's padding rows are addressed too)
        err = "attention_stream_h2: the plane rows of one image (" + std::to_string(ntok) + " tokens x " + std::to_string(heads) +
              " heads) pass 2^31 bytes";
        return false;
    }
    AttStreamH2Plan p;
    p.key_tile = kAttStreamH2KeyTile;
    p.qblock = kAttStreamH2QBlock;
    p.qblocks = (ntok + p.qblock - 1) / p.qblock;
    p.key_tiles = (ntok + p.key_tile - 1) / p.key_tile;
    p.lds_bytes = kAttStreamH2Lds;
    p.wgs_per_cu = kAttStreamH2WgsPerCu;
    const int64_t items = (int64_t)Nimg * heads * p.qblocks;
    if (items > (int64_t)INT32_MAX) {
        err = "attention_stream_h2: " + std::to_string(items) + " work items (Nimg=" + std::to_string(Nimg) + " heads=" + std::to_string(heads) +
              " query blocks=" + std::to_string(p.qblocks) + ")";
        return false;
    }
    p.items = (int)items;
    *plan = p;
    return true;
}

// ---- options table ---------------------------------------------------------------------------------------------------------------------
#define OPT(key, member, rule, a, b, must_be, env, env_fallback) {key, &GemmOptions::member, rule, a, b, must_be, env, env_fallback}
const OptionRow kOptions[] = {
    OPT("gemm_split_k", split_k, kOptAsGiven, 0, 0, nullptr, "RELAX_GEMM_SPLIT", 0),
    OPT("gemm_precision", precision, kOptRange, 0, 3, "0 (fp32), 1 (bf16x3), 2 (bf16x6) or 3 (f16x2)", "RELAX_GEMM_PRECISION", 0),
    OPT("gemm_variant", variant, kOptAsGiven, 0, 0, nullptr, "RELAX_GEMM_VARIANT", 0),
    OPT("gemm_variant_n64", variant_n64, kOptAsGiven, 0, 0, nullptr, "RELAX_GEMM_VARIANT_N64", 0),
    OPT("gemm_group_m", group_m, kOptFloor, 1, 0, nullptr, "RELAX_GEMM_GROUP_M", 0),
    OPT("flow_max_pairs", flow_max_pairs, kOptFloor, 0, 0, nullptr, nullptr, 0),
    OPT("flow_fused", flow_fused, kOptBool, 0, 0, nullptr, nullptr, 0),
    OPT("flow_seg_rows", flow_seg_rows, kOptFloor, 0, 0, nullptr, nullptr, 0),
    OPT("flow_pyramid_fused", flow_pyramid_fused, kOptBool, 0, 0, nullptr, nullptr, 0),
    OPT("x6_fp32_rows", fp32_rows, kOptBool, 0, 0, nullptr, nullptr, 0),
    OPT("rn_h2", rn_h2, kOptBool, 0, 0, nullptr, nullptr, 0),
    OPT("rn_h2_early", rn_h2_early, kOptBool, 0, 0, nullptr, nullptr, 0),
    OPT("rn_fuse", rn_fuse, kOptBool, 0, 0, nullptr, nullptr, 0),
    OPT("rn_c1_h2", rn_c1_h2, kOptBool, 0, 0, nullptr, nullptr, 0),
    OPT("b2b_rows", b2b_rows, kOptOneOf, 128, 256, "128 or 256", nullptr, 0),
    OPT("att_h2", att_h2, kOptBool, 0, 0, nullptr, nullptr, 0),
    OPT("att_h2_stream", att_h2_stream, kOptBool, 0, 0, nullptr, nullptr, 0),
    OPT("h2_form", h2_form, kOptRange, 0, 2, "0, 1 or 2", "RELAX_H2_FORM", 1),
    OPT("h2_stages", h2_stages, kOptOneOf, 3, 4, "3 or 4", nullptr, 0),
    OPT("debug_poison", debug_poison, kOptBool, 0, 0, nullptr, "RELAX_DEBUG_POISON", 0),
};
#undef OPT
const int kNumOptions = (int)(sizeof(kOptions) / sizeof(kOptions[0]));

static const OptionRow* find_option(const char* key) {
    for (const OptionRow& r : kOptions)
        if (std::strcmp(r.key, key) == 0) return &r;
    return nullptr;
}

// the value as the row stores it; false where the row refuses it
static bool option_take(const OptionRow& r, int value, int* stored) {
    switch (r.rule) {
        case kOptAsGiven: *stored = value; return true;
        case kOptBool: *stored = value != 0; return true;
        case kOptFloor: *stored = value > 0 ? value : r.a; return true;
        case kOptOneOf: *stored = value; return value == r.a || value == r.b;
        case kOptRange: *stored = value; return value >= r.a && value <= r.b;
    }
    return false;
}

bool option_set(GemmOptions& o, const char* key, int value, std::string& err) {
    if (!key) {
        err = "relax_set_option: key is NULL";
        return false;
    }
    const OptionRow* r = find_option(key);
    if (!r) {
        err = std::string("relax_set_option: unknown option '") + key + "'";
        return false;
    }
    int stored;
    if (!option_take(*r, value, &stored)) {
        err = std::string("relax_set_option: ") + r->key + " must be " + r->must_be;
        return false;
    }
    o.*(r->member) = stored;
    return true;
}

bool option_get(const GemmOptions& o, const char* key, int* value, std::string& err) {
    if (!key || !value) {
        err = "relax_get_option: NULL argument";
        return false;
    }
    const OptionRow* r = find_option(key);
    if (!r) {
        err = std::string("relax_get_option: unknown option '") + key + "'";
        return false;
    }
    *value = o.*(r->member);
    return true;
}

void options_from_env(GemmOptions& o, const std::function<const char*(const char*)>& lookup) {
    for (const OptionRow& r : kOptions) {
        const char* e = r.env ? lookup(r.env) : nullptr;
        if (!e) continue;
        int stored;
        o.*(r.member) = option_take(r, std::atoi(e), &stored) ? stored : r.env_fallback;
    }
}

// ---- Pillow's 8-bit resample tables ------------------------------------------------------------------------------------------------------
static double filt_bilinear(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}
static double sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}
static double filt_lanczos(double x) { return (-3.0 <= x && x < 3.0) ? sinc(x) * sinc(x / 3) : 0.0; }

constexpr int kResizePrecisionBits = 32 - 8 - 2;

int resize_ksize(int in_size, int out_size, int filt) {
    const double scale = (double)in_size / out_size;
    const double support = (filt == 0 ? 1.0 : 3.0) * (scale < 1.0 ? 1.0 : scale);
    return (int)ceil(support) * 2 + 1;
}

void resize_table(int in_size, int out_size, int filt, int32_t* bounds, int32_t* coeffs) {
    double (*f)(double) = filt == 0 ? filt_bilinear : filt_lanczos;
    const double support0 = filt == 0 ? 1.0 : 3.0;
    const double scale = (double)in_size / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = support0 * filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    std::memset(coeffs, 0, sizeof(int32_t) * (size_t)out_size * ksize);
    const double ss = 1.0 / filterscale;
    std::vector<double> k((size_t)ksize);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        double ww = 0.0;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        for (int x = 0; x < xmax; ++x) {
            const double w = f((x + xmin - center + 0.5) * ss);
            k[x] = w;
            ww += w;
        }
        for (int x = 0; x < xmax; ++x) {
            if (ww != 0.0) k[x] /= ww;
            const double v = k[x];
            coeffs[(size_t)xx * ksize + x] = v < 0 ? (int)(-0.5 + v * (1 << kResizePrecisionBits)) : (int)(0.5 + v * (1 << kResizePrecisionBits));
        }
        bounds[xx * 2] = xmin;
        bounds[xx * 2 + 1] = xmax;
    }
}

bool resize_output_size(int H, int W, int size, int* out_h, int* out_w, std::string& err) {
    char buf[160];
    const char* bad = nullptr;
    int v = 0, lim = kResizeMaxIn;
    if (H < 1 || H > kResizeMaxIn) bad = "H", v = H;
    else if (W < 1 || W > kResizeMaxIn) bad = "W", v = W;
    else if (size < 1 || size > kResizeMaxOut) bad = "size", v = size, lim = kResizeMaxOut;
    if (bad) {
        std::snprintf(buf, sizeof buf, "%s=%d outside 1..%d", bad, v, lim);
        err = buf;
        return false;
    }
    const int64_t shorter = W <= H ? W : H, longer = W <= H ? H : W;
    const int64_t new_long = (int64_t)size * longer / shorter;
    if (new_long > kResizeMaxOut) {
        std::snprintf(buf, sizeof buf, "size=%d makes the longer side %lld of %d x %d, above %d", size, (long long)new_long, H, W, kResizeMaxOut);
        err = buf;
        return false;
    }
    *out_h = W <= H ? (int)new_long : size;
    *out_w = W <= H ? size : (int)new_long;
    return true;
}

bool flow_check_params(double pyr_scale, int levels, int winsize, int iterations, int poly_n, double poly_sigma, int flags, std::string& err) {
    char buf[320];
    buf[0] = 0;
    if (!(pyr_scale >= kFlowMinPyrScale && pyr_scale <= kFlowMaxPyrScale))
        std::snprintf(buf, sizeof buf, "pyr_scale=%g outside %g..%g", pyr_scale, kFlowMinPyrScale, kFlowMaxPyrScale);
    else if (levels < 0 || levels > kFlowMaxLevels)
        std::snprintf(buf, sizeof buf, "levels=%d outside 0..%d", levels, kFlowMaxLevels);
    else if (winsize < kFlowMinWinsize || winsize > kFlowMaxWinsize)
        std::snprintf(buf, sizeof buf, "winsize=%d outside %d..%d", winsize, kFlowMinWinsize, kFlowMaxWinsize);
    else if (winsize % 2 == 0)
        std::snprintf(buf, sizeof buf, "winsize=%d is even: OpenCV's box pass sums 2 * (winsize / 2) + 1 rows and scales by 1 / winsize^2, the "
                      "oracle sums winsize rows, and nothing here can pin which an even window means - odd windows only", winsize);
    else if (iterations < 1 || iterations > kFlowMaxIterations)
        std::snprintf(buf, sizeof buf, "iterations=%d outside 1..%d", iterations, kFlowMaxIterations);
    else if (poly_n != 5 && poly_n != 7)
        std::snprintf(buf, sizeof buf, "poly_n=%d is neither 5 nor 7", poly_n);
    else if (!(std::isfinite(poly_sigma) && poly_sigma > 0))
        std::snprintf(buf, sizeof buf, "poly_sigma=%g is not a finite positive number", poly_sigma);
    else if (flags & 256)
        std::snprintf(buf, sizeof buf, "flags=%d asks for OPTFLOW_FARNEBACK_GAUSSIAN (256): the Gaussian window has no oracle here", flags);
    else if (flags & 4)
        std::snprintf(buf, sizeof buf, "flags=%d asks for OPTFLOW_USE_INITIAL_FLOW (4): an initial flow has no oracle here", flags);
    else if (flags != 0)
        std::snprintf(buf, sizeof buf, "flags=%d: only 0 is accepted", flags);
    if (!buf[0]) return true;
    err = buf;
    return false;
}

bool flow_plan(int H, int W, double pyr_scale, int levels, int* n_levels, FlowLevel* lv, std::string& err) {
    char buf[200];
    buf[0] = 0;
    if (H < 16) std::snprintf(buf, sizeof buf, "H=%d under 16", H);
    else if (W < 16) std::snprintf(buf, sizeof buf, "W=%d under 16", W);
    else if (!(pyr_scale >= kFlowMinPyrScale && pyr_scale <= kFlowMaxPyrScale))
        std::snprintf(buf, sizeof buf, "pyr_scale=%g outside %g..%g", pyr_scale, kFlowMinPyrScale, kFlowMaxPyrScale);
    else if (levels < 0 || levels > kFlowMaxLevels)
        std::snprintf(buf, sizeof buf, "levels=%d outside 0..%d", levels, kFlowMaxLevels);
    if (buf[0]) {
        err = buf;
        return false;
    }
    int used = 0;
    {
        double scale = 1.0;
        for (; used < levels; ++used) {
            scale *= pyr_scale;
            if (W * scale < 32 || H * scale < 32) break;
        }
    }
    for (int k = used; k >= 0; --k) {
        double scale = 1.0;
        for (int i = 0; i < k; ++i) scale *= pyr_scale;
        if (scale < kFlowMinScale) {
            std::snprintf(buf, sizeof buf, "levels=%d at pyr_scale=%g uses scale %g of %d x %d, under 1/32", levels, pyr_scale, scale, H, W);
            err = buf;
            return false;
        }
        FlowLevel& l = lv[used - k];
        l.scale = scale;
        l.sigma = (1. / scale - 1) * 0.5;
        l.ksize = (int)std::lrint(l.sigma * 5) | 1;
        if (l.ksize < 3) l.ksize = 3;
        l.w = (int)std::lrint(W * scale);
        l.h = (int)std::lrint(H * scale);
    }
    *n_levels = used;
    return true;
}

bool flow_gauss_window(int winsize, float* half_taps) {
    if (!half_taps || winsize < kFlowMinWinsize || winsize > kFlowMaxWinsize || winsize % 2 == 0) return false;
    const int m = winsize / 2;
    const double sigma = 0.3 * m;
    double s = 1.0;
    half_taps[0] = 1.f;
    for (int i = 1; i <= m; ++i) {
        half_taps[i] = (float)std::exp(-(double)(i * i) / (2 * sigma * sigma));
        s += 2.0 * half_taps[i];
    }
    s = 1.0 / s;
    for (int i = 0; i <= m; ++i) half_taps[i] = (float)(half_taps[i] * s);
    return true;
}

bool flow_area_table(int src, int dst, int32_t* first, int32_t* count, double* weights) {
    if (!first || !count || !weights || dst < 1 || src < dst) return false;
    const int taps = flow_area_taps(src, dst);
    const double S = (double)src / dst;
    for (int d = 0; d < dst; ++d) {
        const double f1 = d * S, f2 = f1 + S;
        const double cw = std::min(S, src - f1);
        int s1 = (int)std::ceil(f1), s2 = (int)std::floor(f2);
        s2 = std::min(s2, src - 1);
        s1 = std::min(s1, s2);
        double* w = weights + (size_t)d * taps;
        int n = 0, at = s1;
        if (s1 - f1 > 1e-3) {
            at = s1 - 1;
            w[n++] = (s1 - f1) / cw;
        }
        for (int sx = s1; sx < s2; ++sx) w[n++] = 1.0 / cw;
        if (f2 - s2 > 1e-3) w[n++] = std::min(std::min(f2 - s2, 1.0), cw) / cw;
        first[d] = at;
        count[d] = n;
    }
    return true;
}

bool flow_check_params_flags(double pyr_scale, int levels, int winsize, int iterations, int poly_n, double poly_sigma, int flags, std::string& err) {
    if (!flow_check_params(pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, 0, err)) return false;
    if (flags & ~(kFlowFlagInitial | kFlowFlagGaussian)) {
        char buf[400];
        std::snprintf(buf, sizeof buf, "flags=%d has bits outside OPTFLOW_USE_INITIAL_FLOW (4) | OPTFLOW_FARNEBACK_GAUSSIAN (256): %d (those two "
                      "modes are pinned to the formulas stated in relax_hip.h and to float64, not to an OpenCV build; no other mode is restated)",
                      flags, flags & ~(kFlowFlagInitial | kFlowFlagGaussian));
        err = buf;
        return false;
    }
    return true;
}

int flow_chunk_pairs(int H, int W, int64_t ws_gb, int flow_max_pairs, int T) {
    if (H < 1 || W < 1 || T < 1) return 1;      // (refused by the caller; no division by zero on the way there)
    int chunk = (int)((ws_gb << 30) / ((int64_t)H * W * kFlowWsBytesPerPixel));
    if (flow_max_pairs > 0 && chunk > flow_max_pairs) chunk = flow_max_pairs;   // tests: force the chunk loop
    if (chunk < 1) chunk = 1;
    return chunk > T ? T : chunk;
}

// Long segments keep the window's warm-up rows (and their re-read operands) small; shorter ones when the level is small, so that a clip's 32
// pairs still give every CU work: 18, 9, 6, 4, 3 or 2 windows (270 .. 30 rows at 15, the ring period of the register-ring kernels).
int flow_segment_rows(int seg_rows, int bands, int h, int winsize) {
    if (seg_rows > 0) return (seg_rows + winsize - 1) / winsize * winsize;
    for (const int mult : {18, 9, 6, 4, 3})
        if (bands * ((h + mult * winsize - 1) / (mult * winsize)) >= 16) return mult * winsize;
    return 2 * winsize;
}

bool flow_schedule(const FlowParams& fp, const FlowRequest& rq, const FlowOptions& o, FlowSchedule* sc, std::string& err) {
    const int H = rq.H, W = rq.W, P = rq.P;
    FlowLevel plan[kFlowMaxLevels + 1];
    int levels = 0;
    if (!flow_plan(H, W, fp.pyr_scale, fp.levels, &levels, plan, err)) return false;
    const int64_t HW = (int64_t)H * W;
    char buf[200];
    auto refuse = [&]() {
        err = buf;
        return false;
    };
    // the matrix kernels address a pair's two coefficient images through ONE buffer resource with 32-bit byte offsets
    if (HW * 40 >= (int64_t)0x7fffffff) {
        std::snprintf(buf, sizeof buf, "frames of %d x %d exceed the 2 GB a buffer resource addresses (40 bytes per pixel)", W, H);
        return refuse();
    }
    const bool gaussian = (fp.flags & kFlowFlagGaussian) != 0;
    float taps[kFlowMaxHalfWindow + 1];
    if (gaussian && !flow_gauss_window(fp.winsize, taps)) {
        std::snprintf(buf, sizeof buf, "no Gaussian window of %d", fp.winsize);
        return refuse();
    }
    *sc = FlowSchedule{};
    sc->n_levels = levels;
    sc->iterations = fp.iterations;
    // the arena, all regions sized for level 0
    const int64_t plane = (int64_t)P * 2 * HW;       // [P][2][H][W], or a flow [P][H][W][2]
    sc->gray_off = 0;
    sc->tmp_off = plane;
    sc->blur_off = 2 * plane;
    sc->I_off = 3 * plane;
    sc->R_off = 4 * plane;                           // [P][2][h][w][5]
    sc->M_off = sc->R_off + (int64_t)P * 10 * HW;    // [P][h][w][5]
    sc->flow_off[0] = sc->M_off + (int64_t)P * 5 * HW;
    sc->flow_off[1] = sc->flow_off[0] + plane;
    sc->mm_off = sc->flow_off[1] + plane;
    sc->arena_bytes = (HW * kFlowArenaFloatsPerPixel * (int64_t)sizeof(float) + 16) * P;
    // the four level inputs in one pass over the frames when the scales are exact: blur -> level 0, I -> level 1, tmp -> levels 2 and 3
    const bool pyr = o.pyramid_fused && levels == 3 && fp.pyr_scale == 0.5 && H % 8 == 0 && W % 8 == 0 && rq.stride4 && rq.frames4;
    sc->pyr_off[0] = sc->blur_off;
    sc->pyr_off[1] = sc->I_off;
    sc->pyr_off[2] = sc->tmp_off;
    sc->pyr_off[3] = sc->tmp_off + (int64_t)P * 2 * (HW / 16);
    sc->gray = pyr ? kFlowGrayNone : (HW % 4 == 0 && rq.stride4 && rq.frames4 && rq.arena16 ? kFlowGrayV4 : kFlowGray);
    // bytes: the frames once and the four level inputs once | the frames read, the gray plane written
    sc->bytes = pyr ? 2.0 * P * HW * (3 + 4 * (1 + 0.25 + 0.0625 + 0.015625)) : 2.0 * P * HW * (3 + 4);

    int cur = 0, prev = -1, ph = 0, pw = 0;          // the buffer the level starts in; the coarser level's result and its size
    for (int k = levels; k >= 0; --k) {
        FlowLevelPlan& L = sc->lvl[levels - k];
        L.lv = plan[levels - k];
        const double scale = L.lv.scale;
        const int smooth = L.lv.ksize, w = L.lv.w, hh = L.lv.h;
        const int64_t hw = (int64_t)w * hh;
        // coarse levels (scale < 1/2) blur only where the resize samples; past kFlowMaxGauss taps, or a row stage past kFlowGhSeg floats
        // (scales under 1/8), the wide instantiations of the same kernels
        const bool sampled = scale < 0.5;
        const bool wide = smooth > kFlowMaxGauss || (sampled && 129.0 * W / w + smooth + 4 > kFlowGhSeg);
        if (smooth >= kFlowMaxGaussWide) {
            std::snprintf(buf, sizeof buf, "smoothing kernel %d too large", smooth);
            return refuse();
        }
        if (sampled && 129.0 * W / w + smooth + 4 > kFlowGhSegWide) {
            std::snprintf(buf, sizeof buf, "pyramid scale %g too coarse for the row stage", scale);
            return refuse();
        }
        if (wide && !sampled) {      // (scale >= 1/2 has 3 taps)
            std::snprintf(buf, sizeof buf, "%d smoothing taps at scale %g", smooth, scale);
            return refuse();
        }
        if (pyr && smooth != (k < 2 ? 3 : (k == 2 ? 9 : 19))) {      // PyramidTaps holds 3, 3, 9 and 19
            std::snprintf(buf, sizeof buf, "unexpected smoothing kernel %d at level %d", smooth, k);
            return refuse();
        }
        L.start = cur;
        L.up = prev < 0 ? (rq.have_init ? kFlowUpArea : kFlowUpZeros) : (fp.pyr_scale == 0.5 ? kFlowUpFusedX2 : kFlowUpResize);
        if (L.up == kFlowUpArea) L.bytes += 8.0 * P * ((double)HW + (double)hw);
        if (L.up == kFlowUpResize) L.bytes += 8.0 * P * ((double)ph * pw + (double)hw);
        if (pyr) L.pyramid = kFlowPyrFused;
        else if (sampled) L.pyramid = wide ? kFlowPyrSampledWide : kFlowPyrSampled;
        else L.pyramid = smooth == 3 && W % 4 == 0 && HW % 4 == 0 && rq.arena16 ? kFlowPyrGauss3V4 : kFlowPyrGaussPass;   // (blur_off is whole 16 bytes)
        L.resize = !pyr && !sampled && (w != W || hh != H);
        if (!pyr)   // the gray frame read once, the level input written once (+ the full-size blur written and read below full size)
            L.bytes += 2.0 * P * (4.0 * HW + 4.0 * hw + (k >= 1 && !sampled ? 8.0 * HW : 0.0));
        L.poly_n = fp.poly_n;
        L.poly_bands = (w + flow_poly_band(fp.poly_n) - 1) / flow_poly_band(fp.poly_n);
        L.poly_seg = 64;   // a ring of rows to fill before the first one; shorter segments when the level is small (enough blocks for 256 CUs)
        while (L.poly_seg > 16 && (int64_t)L.poly_bands * ((hh + L.poly_seg - 1) / L.poly_seg) * P * 2 < 2048) L.poly_seg -= 16;
        L.bytes += 2.0 * P * hw * 24;      // 4 bytes in, 5 coefficients out per pixel and frame
        // the fused iteration kernel is written for the 15-pixel box window (its ring, its fill steps); every other window takes two kernels
        L.iteration = o.fused && fp.winsize == kFlowWinsize && !gaussian ? kFlowItFused
                      : (gaussian ? kFlowItGaussAny : (fp.winsize == kFlowWinsize ? kFlowItBoxFused : kFlowItBoxAny));
        if (L.iteration == kFlowItGaussAny) {
            L.out_cols = kFlowGaussTileW;
            L.seg = kFlowGaussTileH;
        } else {
            L.out_cols = flow_box_band(fp.winsize);
            L.seg = flow_segment_rows(o.seg_rows, (w + L.out_cols - 1) / L.out_cols, hh, fp.winsize);
        }
        L.bands = (w + L.out_cols - 1) / L.out_cols;
        L.segments = (hh + L.seg - 1) / L.seg;
        L.um_gx = (w + 255) / 256;
        L.um_rows = (hh + 7) / 8;
        // per pixel: flow_iteration - 2 x 5 floats of R at the pixel and at the displaced position (counted once: neighbours share the lines) +
        // the flow in and out = 56 bytes; update_matrices_k - the same 40 + 8 (flow) + 20 (M written) = 68, and the solve's 28: M read, flow written
        const bool fused = L.iteration == kFlowItFused;
        L.it_bytes = (fused ? 56.0 : 68.0) * (double)hw * P;
        L.bytes += fp.iterations * (fused ? L.it_bytes : L.it_bytes + 28.0 * (double)hw * P);
        int in = L.up == kFlowUpFusedX2 ? prev : cur, out = fused && L.up != kFlowUpFusedX2 ? 1 - cur : cur;
        for (int it = 0; it < fp.iterations; ++it) {
            L.step[it] = FlowStep{in, out, k == 0 && it == fp.iterations - 1 && rq.want_image};
            in = out;
            if (fused) out = 1 - out;
        }
        prev = in;       // the level's result
        ph = hh;
        pw = w;
        cur = 1 - prev;
        sc->bytes += L.bytes;
    }
    sc->result = prev;
    if (rq.want_image) sc->bytes += 11.0 * P * HW;      // the flow read, 3 bytes per pixel written
    return true;
}

}  // namespace host
}  // namespace relax

#ifdef RELAX_FLOW_FLAGS_MAIN
// ---- stand-alone program (make flow_flags_san: AddressSanitizer + UBSan, CPU only): the Gaussian window of every odd winsize and the area table of
// a grid of (src, dst) into heap arrays of exactly the stated sizes; taps sum to 1 +- 1e-6, every table index in range, rows sum to 1 +- 1e-12 -
// except where the definition itself drops an overlap of at most 1e-3 pixel (possible only when dst / gcd(src, dst) >= 1000: the fractional parts
// of d * src / dst are multiples of gcd / dst), where a row may fall short of 1 by at most 2e-3 / cw ---------------------------------------------
static int flags_gcd(int a, int b) { return b ? flags_gcd(b, a % b) : a; }
int main() {
    using namespace relax::host;
    long windows = 0, tables = 0, short_tables = 0;
    for (int ws = kFlowMinWinsize; ws <= kFlowMaxWinsize; ws += 2) {
        std::vector<float> k((size_t)ws / 2 + 1);
        if (!flow_gauss_window(ws, k.data())) return 1;
        double sum = k[0];
        for (int i = 1; i <= ws / 2; ++i) {
            sum += 2.0 * k[i];
            if (!(k[i] > 0 && k[i] < k[i - 1])) {
                std::printf("winsize %d: tap %d not positive and decreasing\n", ws, i);
                return 1;
            }
        }
        if (std::fabs(sum - 1.0) > 1e-6) {
            std::printf("winsize %d: taps sum to %.9f\n", ws, sum);
            return 1;
        }
        ++windows;
    }
    float none[1];
    if (flow_gauss_window(14, none) || flow_gauss_window(65, none) || flow_gauss_window(1, none)) return 1;
    std::vector<int> sides;
    for (int n = 16; n <= 2200; n += 53) sides.push_back(n);
    for (int n : {31, 32, 33, 48, 66, 78, 97, 105, 131, 256, 264, 1000, 1001, 1080, 1920, 2160, 2199, 2200}) sides.push_back(n);
    for (int src : sides)
        for (int dst : sides) {
            if (dst > src) continue;
            const int taps = flow_area_taps(src, dst);
            std::vector<int32_t> first((size_t)dst), count((size_t)dst);
            std::vector<double> w((size_t)dst * taps);
            if (!flow_area_table(src, dst, first.data(), count.data(), w.data())) return 1;
            const bool may_drop = dst / flags_gcd(src, dst) >= 1000;
            const double S = (double)src / dst;
            for (int d = 0; d < dst; ++d) {
                double sum = 0;
                for (int j = 0; j < count[d]; ++j) sum += w[(size_t)d * taps + j];
                const double cw = std::min(S, src - d * S);
                const bool ok = count[d] >= 1 && count[d] <= taps && first[d] >= 0 && first[d] + count[d] <= src &&
                                (may_drop ? sum <= 1 + 1e-12 && sum >= 1 - 2e-3 / cw - 1e-12 : std::fabs(sum - 1.0) <= 1e-12);
                if (!ok) {
                    std::printf("bad area row %d of %d -> %d: first %d, count %d, sum %.17g\n", d, src, dst, first[d], count[d], sum);
                    return 1;
                }
            }
            ++tables;
            short_tables += may_drop;
        }
    int32_t i1[1];
    double d1[4];
    if (flow_area_table(16, 17, i1, i1, d1) || flow_area_table(16, 0, i1, i1, d1)) return 1;
    std::string err;
    for (int fl : {0, 4, 256, 260})
        if (!flow_check_params_flags(0.5, 3, 15, 3, 5, 1.2, fl, err)) return 1;
    for (int fl : {1, 2, 8, 261, 512, -1})
        if (flow_check_params_flags(0.5, 3, 15, 3, 5, 1.2, fl, err) || err.find("flags=") == std::string::npos) return 1;
    if (flow_check_params_flags(0.5, 3, 14, 3, 5, 1.2, 256, err) || err.find("winsize=14") == std::string::npos) return 1;
    std::printf("flow_flags ok: %ld windows, %ld area tables (%ld of them may drop an overlap under 1e-3)\n", windows, tables, short_tables);
    return 0;
}
#endif

#ifdef RELAX_FLOW_PLAN_MAIN
// ---- stand-alone program (make flow_plan_san: AddressSanitizer + UBSan, CPU only): every plan of a grid of sizes, scales and depths into a heap
// array of exactly kFlowMaxLevels + 1 entries, its invariants checked, and eight schedules of it into heap structs; every refusal of flow_check_params once ---------------------------------
int main() {
    using namespace relax::host;
    const double scales[] = {0.5, 0.6, 0.7, 0.75, 0.8, 0.9, 0.95};
    long plans = 0, refused = 0, schedules = 0;
    std::string err;
    for (int H = 16; H <= 2200; H += 37)
        for (int W = 16; W <= 4200; W += 211)
            for (double ps : scales)
                for (int levels = 0; levels <= kFlowMaxLevels; ++levels) {
                    std::vector<FlowLevel> lv((size_t)kFlowMaxLevels + 1);
                    int n = -1;
                    if (!flow_plan(H, W, ps, levels, &n, lv.data(), err)) {
                        ++refused;
                        continue;
                    }
                    ++plans;
                    bool ok = n >= 0 && n <= levels && lv[n].h == H && lv[n].w == W && lv[n].ksize == 3 && lv[n].sigma == 0;
                    for (int i = 0; i <= n && ok; ++i)
                        ok = lv[i].ksize >= 3 && lv[i].ksize <= kFlowMaxTaps && lv[i].ksize % 2 == 1 && lv[i].scale >= kFlowMinScale &&
                             (i == n || (lv[i].h >= 32 && lv[i].w >= 32 && lv[i].h <= lv[i + 1].h && lv[i].w <= lv[i + 1].w));
                    if (!ok) {
                        std::printf("bad plan for %d x %d, pyr_scale %g, levels %d\n", H, W, ps, levels);
                        return 1;
                    }
                    // the schedule of the same plan into a heap struct of exactly its size: both windows' kinds, both flag bits, every option
                    for (int v = 0; v < 8; ++v) {
                        const FlowParams fp{ps, levels, v & 1 ? 15 : 63, v & 2 ? 10 : 1, v & 4 ? 7 : 5, 1.2, (v & 1 ? 0 : kFlowFlagGaussian) | (v & 2 ? kFlowFlagInitial : 0)};
                        const FlowRequest rq{H, W, v & 4 ? 32 : 1, v & 1, 1, v & 2 ? 1 : 0, (v >> 1) & 1, 1, v & 1};
                        const FlowOptions o{v & 1, (v >> 2) & 1, v == 7 ? 40 : 0};
                        std::unique_ptr<FlowSchedule> sc(new FlowSchedule);
                        if (!flow_schedule(fp, rq, o, sc.get(), err)) {
                            std::printf("no schedule for %d x %d, pyr_scale %g, levels %d: %s\n", H, W, ps, levels, err.c_str());
                            return 1;
                        }
                        const FlowLevelPlan& l0 = sc->lvl[sc->n_levels];
                        ++schedules;
                        if (sc->n_levels != n || l0.lv.h != H || l0.step[fp.iterations - 1].out != sc->result || sc->arena_bytes <= 0 || !(sc->bytes > 0)) {
                            std::printf("bad schedule for %d x %d, pyr_scale %g, levels %d\n", H, W, ps, levels);
                            return 1;
                        }
                    }
                }
    const struct { double ps; int lv, ws, it, pn; double sg; int fl; } bad[] = {
        {0.49, 3, 15, 3, 5, 1.2, 0}, {1.0, 3, 15, 3, 5, 1.2, 0}, {0.5, 9, 15, 3, 5, 1.2, 0}, {0.5, 3, 14, 3, 5, 1.2, 0}, {0.5, 3, 65, 3, 5, 1.2, 0},
        {0.5, 3, 15, 0, 5, 1.2, 0}, {0.5, 3, 15, 3, 6, 1.2, 0}, {0.5, 3, 15, 3, 5, 0.0, 0}, {0.5, 3, 15, 3, 5, NAN, 0}, {0.5, 3, 15, 3, 5, 1.2, 4},
        {0.5, 3, 15, 3, 5, 1.2, 256}, {0.5, 3, 15, 3, 5, 1.2, 1}};
    for (const auto& b : bad)
        if (flow_check_params(b.ps, b.lv, b.ws, b.it, b.pn, b.sg, b.fl, err) || err.empty()) {
            std::printf("not refused: %g %d %d %d %d %g %d\n", b.ps, b.lv, b.ws, b.it, b.pn, b.sg, b.fl);
            return 1;
        }
    if (!flow_check_params(0.5, 3, 15, 3, 5, 1.2, 0, err) || !flow_check_params(0.95, 8, 63, 10, 7, 0.1, 0, err)) return 1;
    std::printf("flow_plan ok: %ld plans, %ld refused, %ld schedules\n", plans, refused, schedules);
    return 0;
}
#endif

#ifdef RELAX_HOST_TEST_API
// ---- C entry points of the host half alone (librelax_host_san.so of tests/test_host_logic_sanitized.py; compiled only
// with -DRELAX_HOST_TEST_API: the product library does not export them) ---------------------------------------------------------------------------------
extern "C" {

// 0 and the folded / packed weights if every key is present with the right size; -1 and a message otherwise.
// out must hold cout * conv_kpad(k, cin_pad) floats, shift cout floats (shift may be NULL when bn is NULL).
int relax_host_pack_conv(const float* const* tensors, const char* const* names, const int64_t* numels, int n, const char* conv,
                         const char* bn, int cout, int cin, int cin_pad, int k, float* out, float* shift, char* err, int err_len) {
    using namespace relax::host;
    StateDict sd;
    for (int i = 0; i < n; ++i) sd.add(names[i], tensors[i], numels[i]);
    std::string e;
    auto fail = [&]() {
        if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s", e.c_str());
        return -1;
    };
    const std::string c(conv);
    const float* w = sd.get(c + ".weight", (int64_t)cout * cin * k * k, e);
    if (!w) return fail();
    float* scale = nullptr;
    std::vector<float> storage;
    if (bn && *bn) {
        storage.resize((size_t)cout);
        scale = storage.data();
        if (!read_bn(sd, bn, cout, 1e-5f, scale, shift, e)) return fail();
    }
    pack_conv_oihw(w, scale, cout, cin, cin_pad, k, conv_kpad(k, cin_pad), out);
    return 0;
}

// the BatchNorm under `prefix` folded into scale / shift [channels]: 0, or -1 and the message naming the missing / mis-sized key
int relax_host_read_bn(const float* const* tensors, const char* const* names, const int64_t* numels, int n, const char* prefix, int channels,
                       float eps, float* scale, float* shift, char* err, int err_len) {
    relax::host::StateDict sd;
    for (int i = 0; i < n; ++i) sd.add(names[i], tensors[i], numels[i]);
    std::string e;
    if (relax::host::read_bn(sd, prefix, channels, eps, scale, shift, e)) return 0;
    if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s", e.c_str());
    return -1;
}

void relax_host_fold_bn(const float* gamma, const float* beta, const float* mean, const float* var, float eps, int channels, float* scale, float* shift) {
    relax::host::fold_bn(gamma, beta, mean, var, eps, channels, scale, shift);
}

void relax_host_conv_hoelder(const float* rows, const float* bias_or_null, int cout, int k, float* l1max, float* bmax) {
    relax::host::conv_hoelder(rows, bias_or_null, cout, k, l1max, bmax);
}

int relax_host_conv_kpad(int k, int cin_pad) { return relax::host::conv_kpad(k, cin_pad); }

int relax_host_fold_fc_bn(const float* const* tensors, const char* const* names, const int64_t* numels, int n, int f, int fpad,
                          float* w1p, float* b1p, int* h1_out, char* err, int err_len) {
    using namespace relax::host;
    StateDict sd;
    for (int i = 0; i < n; ++i) {
        if (names[i] && std::string(names[i]) == "n_averaged") continue;
        sd.add(names[i], tensors[i], numels[i], true);
    }
    std::string e;
    auto fail = [&]() {
        if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s", e.c_str());
        return -1;
    };
    const int64_t nw = sd.numel("fc1.weight");
    if (nw <= 0 || f <= 0 || nw % f != 0) {
        e = "mlp head: fc1.weight missing or not [hidden, input_features]";
        return fail();
    }
    const int h1 = (int)(nw / f);
    if (h1_out) *h1_out = h1;
    if (!w1p) return 0;   // size query
    const float* w1 = sd.get("fc1.weight", nw, e, "mlp head state dict");
    const float* b1 = w1 ? sd.get("fc1.bias", h1, e, "mlp head state dict") : nullptr;
    const float* g = b1 ? sd.get("bn1.weight", h1, e, "mlp head state dict") : nullptr;
    const float* be = g ? sd.get("bn1.bias", h1, e, "mlp head state dict") : nullptr;
    const float* mu = be ? sd.get("bn1.running_mean", h1, e, "mlp head state dict") : nullptr;
    const float* var = mu ? sd.get("bn1.running_var", h1, e, "mlp head state dict") : nullptr;
    if (!var) return fail();
    fold_fc_bn(w1, b1, g, be, mu, var, 1e-5f, h1, f, fpad, w1p, b1p);
    return 0;
}

void relax_host_tail_split(int ntiles, int slots, int nk, int min_steps, int can_split, int* full_tiles, int* nsplit) {
    const relax::host::TailSplit r = relax::host::choose_tail_split(ntiles, slots, nk, min_steps, can_split != 0);
    if (full_tiles) *full_tiles = r.full_tiles;
    if (nsplit) *nsplit = r.nsplit;
}

// the f16x2 scale helpers (csrc/h2.h): scales[rows], and the two bounds
void relax_host_h2_weight_row_scales(const float* w, int rows, int k, float* scale) { relax::host::h2_weight_row_scales(w, rows, k, scale); }
float relax_host_h2_scale_for_bound(double amax) { return relax::host::h2_scale_for_bound(amax); }
double relax_host_layernorm_out_bound(const float* gamma, const float* beta, int dim) { return relax::host::layernorm_out_bound(gamma, beta, dim); }
double relax_host_linear_of_layernorm_bound(const float* w, const float* b, const float* gamma, const float* beta, int dim, int n0, int n1) {
    return relax::host::linear_of_layernorm_bound(w, b, gamma, beta, dim, n0, n1);
}

// VGG-16: 0 if every key is present with its size, -1 and the message otherwise; and the fc1 column permutation
int relax_host_vgg16_check_keys(const float* const* tensors, const char* const* names, const int64_t* numels, int n, char* err, int err_len) {
    relax::host::StateDict sd;
    for (int i = 0; i < n; ++i) sd.add(names[i], tensors[i], numels[i]);
    std::string e;
    if (relax::host::vgg16_check_keys(sd, e)) return 0;
    if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s", e.c_str());
    return -1;
}
void relax_host_vgg16_fc1_to_nhwc(const float* w, int rows, int c, int hw, float* out) { relax::host::vgg16_fc1_to_nhwc(w, rows, c, hw, out); }
// VGG-16 schedule as plain integers.  opts: precision; req: N, want_layer_stack, want_pool, tap mask.  out: [n_slots, classifier, n_rows] + per step
// the 16 VggLayerPlan fields in declaration order + per convolution [map side, pool behind it] (3 + 20 * 16 + 13 * 2 ints); arena: the eight
// VggArena offsets + vgg_arena_bytes(N).  0, or -1 with a message and both arrays untouched when the plan needs more than max_slots slots.
int relax_host_vgg_plan(const int* opts, const int* req, int max_slots, int* out, int64_t* arena, char* err, int err_len) {
    using namespace relax::host;
    static_assert(sizeof(VggLayerPlan) == 16 * sizeof(int) && sizeof(VggArena) == 8 * sizeof(int64_t), "VggLayerPlan is 16 ints, VggArena 8 offsets");
    VggPlan p;
    std::string e;
    if (!vgg_plan(VggOptions{opts[0]}, VggRequest{req[0], req[1], req[2], (unsigned)req[3]}, max_slots, &p, e)) {
        if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s", e.c_str());
        return -1;
    }
    out[0] = p.n_slots; out[1] = p.classifier; out[2] = p.n_rows;
    std::memcpy(out + 3, p.row, sizeof(p.row));
    int* geo = out + 3 + kVggSteps * 16;
    for (int i = 0; i < kVggConvs; ++i) {
        geo[2 * i] = kVggConvSide[i];
        geo[2 * i + 1] = kVggPoolAfter[i];
    }
    std::memcpy(arena, &p.arena, sizeof(p.arena));
    arena[8] = vgg_arena_bytes(req[0]);
    return 0;
}

// ResNet-50 schedule as plain integers.  opts: the six RnOptions in order; req: N, n_ls, pool_from, want_pool, tap mask.
// out: [conv1_h2, pool_f32, s_stem, n_slots] + per block the 23 RnBlockPlan fields in declaration order (4 + 16 * 23 ints).
// 0, or -1 with a message and `out` untouched when the plan needs more than max_slots slots.
int relax_host_rn_plan(const int* opts, const int* req, int max_slots, int* out, char* err, int err_len) {
    using namespace relax::host;
    static_assert(sizeof(RnBlockPlan) == 23 * sizeof(int), "RnBlockPlan is 23 ints");
    const RnOptions o{opts[0], opts[1], opts[2], opts[3], opts[4], opts[5]};
    const RnRequest rq{req[0], req[1], req[2], req[3], (unsigned)req[4]};
    RnPlan p;
    std::string e;
    if (!rn_plan(o, rq, max_slots, &p, e)) {
        if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s", e.c_str());
        return -1;
    }
    static_assert(sizeof(RnPlan) == (4 + kRnBlocks * 23) * sizeof(int), "RnPlan is a flat array of ints");
    std::memcpy(out, &p, sizeof(p));
    return 0;
}
// Farneback schedule as plain numbers.  par: pyr_scale, poly_sigma; ipar: levels, winsize, iterations, poly_n, flags; req: the nine FlowRequest
// fields in order; opts: the three FlowOptions.  iout: [n_levels, iterations, gray, result, the 9 offsets gray .. mm, pyr_off[4], arena_bytes]
// (18) + per level, coarsest first, 9 levels: [h, w, ksize, pyramid, resize, up, start, poly_n, poly_bands, poly_seg, iteration, bands, out_cols,
// seg, segments, um_gx, um_rows] + 10 steps x [in, out, minmax] (47).  dout: [bytes] + per level [scale, sigma, it_bytes, bytes].
// 0, or -1 with the message and both arrays untouched.
int relax_host_flow_schedule(const double* par, const int* ipar, const int* req, const int* opts, int64_t* iout, double* dout, char* err,
                             int err_len) {
    using namespace relax::host;
    const FlowParams fp{par[0], ipar[0], ipar[1], ipar[2], ipar[3], par[1], ipar[4]};
    const FlowRequest rq{req[0], req[1], req[2], req[3], req[4], req[5], req[6], req[7], req[8]};
    const FlowOptions o{opts[0], opts[1], opts[2]};
    FlowSchedule sc;
    std::string e;
    if (!flow_schedule(fp, rq, o, &sc, e)) {
        if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s", e.c_str());
        return -1;
    }
    const int64_t head[18] = {sc.n_levels, sc.iterations, sc.gray, sc.result, sc.gray_off, sc.tmp_off, sc.blur_off, sc.I_off, sc.R_off, sc.M_off,
                              sc.flow_off[0], sc.flow_off[1], sc.mm_off, sc.pyr_off[0], sc.pyr_off[1], sc.pyr_off[2], sc.pyr_off[3], sc.arena_bytes};
    std::memcpy(iout, head, sizeof head);
    dout[0] = sc.bytes;
    for (int i = 0; i <= kFlowMaxLevels; ++i) {
        const FlowLevelPlan& L = sc.lvl[i];
        const int v[17] = {L.lv.h, L.lv.w, L.lv.ksize, L.pyramid, L.resize, L.up, L.start, L.poly_n, L.poly_bands, L.poly_seg, L.iteration, L.bands,
                           L.out_cols, L.seg, L.segments, L.um_gx, L.um_rows};
        int64_t* p = iout + 18 + i * 47;
        for (int j = 0; j < 17; ++j) p[j] = v[j];
        for (int j = 0; j < kFlowMaxIterations; ++j) {
            p[17 + 3 * j] = L.step[j].in;
            p[18 + 3 * j] = L.step[j].out;
            p[19 + 3 * j] = L.step[j].minmax;
        }
        const double d[4] = {L.lv.scale, L.lv.sigma, L.it_bytes, L.bytes};
        std::memcpy(dout + 1 + 4 * i, d, sizeof d);
    }
    return 0;
}
int relax_host_flow_chunk_pairs(int H, int W, int64_t ws_gb, int flow_max_pairs, int T) {
    return relax::host::flow_chunk_pairs(H, W, ws_gb, flow_max_pairs, T);
}
// the 16 bottlenecks: block, layer, index, cin, width, cout, stride, has_down, tap (16 * 9 ints)
// the canvas entries under canvas flags (kRnCanvasAny; 0: the default rule and its messages)
int relax_host_rn_canvas_geometry_ex(int Hc, int Wc, int flags, int* tap_hw, int64_t* sizes, char* err, int err_len) {
    relax::host::RnCanvasGeometry g;
    std::string e;
    if (!relax::host::rn_canvas_geometry(Hc, Wc, flags, &g, e)) {
        if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s", e.c_str());
        return -1;
    }
    if (tap_hw) std::memcpy(tap_hw, g.tap_hw, sizeof(g.tap_hw));
    if (sizes) {
        const int64_t v[8] = {g.x0, g.big, g.t1, g.t2, g.gap_ws, g.block_max, g.floats_f32, g.floats_x6};
        std::memcpy(sizes, v, sizeof(v));
    }
    return 0;
}
int relax_host_rn_plan_canvas_ex(const int* opts, const int* req, int Hc, int Wc, int flags, int max_slots, int* out, char* err, int err_len) {
    using namespace relax::host;
    const RnOptions o{opts[0], opts[1], opts[2], opts[3], opts[4], opts[5]};
    const RnRequest rq{req[0], req[1], req[2], req[3], (unsigned)req[4]};
    RnCanvas cv;
    cv.Hc = Hc; cv.Wc = Wc; cv.flags = flags;
    RnPlan p;
    std::string e;
    if (!rn_plan(o, rq, cv, max_slots, &p, e)) {
        if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s", e.c_str());
        return -1;
    }
    std::memcpy(out, &p, sizeof(p));
    return 0;
}
// the same on an [Hc, Wc] canvas; a refused canvas: -1 and rn_canvas_geometry's message
int relax_host_rn_plan_canvas(const int* opts, const int* req, int Hc, int Wc, int max_slots, int* out, char* err, int err_len) {
    return relax_host_rn_plan_canvas_ex(opts, req, Hc, Wc, 0, max_slots, out, err, err_len);
}
// canvas geometry: tap_hw [15][2]; sizes = x0, big, t1, t2, gap_ws, block_max, floats_f32, floats_x6 (8 values).  0, or -1 and the message
int relax_host_rn_canvas_geometry(int Hc, int Wc, int* tap_hw, int64_t* sizes, char* err, int err_len) {
    return relax_host_rn_canvas_geometry_ex(Hc, Wc, 0, tap_hw, sizes, err, err_len);
}
// the launches in front of the blocks: out = stem_form, pool_form, stem_fused_mean
int relax_host_rn_stem_plan_ex(int Hc, int Wc, int flags, int* out, char* err, int err_len) {
    using namespace relax::host;
    RnCanvas cv;
    cv.Hc = Hc; cv.Wc = Wc; cv.flags = flags;
    RnStemPlan p;
    std::string e;
    if (!rn_stem_plan(cv, &p, e)) {
        if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s", e.c_str());
        return -1;
    }
    std::memcpy(out, &p, sizeof(p));
    return 0;
}
void relax_host_rn_geometry(int* out) { std::memcpy(out, relax::host::rn_geometry(), sizeof(relax::host::RnBlockGeom) * relax::host::kRnBlocks); }

// ViT geometry: out = patch, side, npatch, ntok, patch_k; 0, or -1 and a message.  Arena floats per image: out[0] fp32 layout, out[1] bf16x6 layout.
int relax_host_vit_geometry(int patch, int* out, char* err, int err_len) {
    relax::host::VitGeometry g;
    std::string e;
    if (!relax::host::vit_geometry(patch, &g, e)) {
        if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s", e.c_str());
        return -1;
    }
    std::memcpy(out, &g, sizeof(g));
    return 0;
}
// the grid of a call: out = gh, gw, npatch, ntok, identity; 0, or -1 and a message
int relax_host_vit_canvas_geometry(int patch, int Hc, int Wc, int* out, char* err, int err_len) {
    relax::host::VitCanvasGeometry g;
    std::string e;
    if (!relax::host::vit_canvas_geometry(patch, Hc, Wc, &g, e)) {
        if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s", e.c_str());
        return -1;
    }
    std::memcpy(out, &g, sizeof(g));
    return 0;
}
// one axis of the position table's bicubic resampling: idx[4 g], w[4 g]
void relax_host_pos_interp_taps(int side, int g, int32_t* idx, float* w) { relax::host::pos_interp_taps(side, g, idx, w); }
void relax_host_vit_arena_floats(int dim, int ntok, int npatch, int patch_k, int64_t* out) {
    out[0] = relax::host::vit_arena(false, dim, ntok, npatch, patch_k).floats;
    out[1] = relax::host::vit_arena(true, dim, ntok, npatch, patch_k).floats;
}
// the forward's plan.  in = precision, att_h2, att_h2_stream | dim, depth, heads, patch, patch_k | ntok, npatch, want_tokens, want_pooled,
// want_cls_attention, n_last; out = arith, patch_embed, qkv_planes, attention, attention_only, final_norm, then the arena's eight offsets
void relax_host_vit_plan(const int* in, int64_t* out) {
    using namespace relax::host;
    const VitPlan p = vit_plan(VitOptions{in[0], in[1], in[2]}, VitModel{in[3], in[4], in[5], in[6], in[7]},
                               VitRequest{in[8], in[9], in[10], in[11], in[12], in[13]});
    const int64_t v[14] = {p.arith, p.patch_embed, p.qkv_planes, p.attention, p.attention_only, p.final_norm, p.arena.patches, p.arena.embedded,
                           p.arena.residual, p.arena.operand, p.arena.qkv, p.arena.final, p.arena.hidden, p.arena.floats};
    std::memcpy(out, v, sizeof(v));
}
// streaming-attention plan: out = qblock, qblocks, key_tiles, lds_bytes, items; 0, or -1 and a message
int relax_host_att_stream_plan(int Nimg, int heads, int ntok, int arith, int* out, char* err, int err_len) {
    relax::host::AttStreamPlan p;
    std::string e;
    if (!relax::host::att_stream_plan(Nimg, heads, ntok, arith, &p, e)) {
        if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s", e.c_str());
        return -1;
    }
    std::memcpy(out, &p, sizeof(p));
    return 0;
}
// f16x2 streaming-attention plan: out = key_tile, qblock, qblocks, key_tiles, lds_bytes, wgs_per_cu, items; 0, or -1 and a message
int relax_host_att_stream_h2_plan(int Nimg, int heads, int ntok, int* out, char* err, int err_len) {
    relax::host::AttStreamH2Plan p;
    std::string e;
    if (!relax::host::att_stream_h2_plan(Nimg, heads, ntok, &p, e)) {
        if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s", e.c_str());
        return -1;
    }
    std::memcpy(out, &p, sizeof(p));
    return 0;
}

// the options table.  The i-th key (NULL past the end); a GemmOptions with its defaults on the heap; set / get by key: 0, or -1 and the
// message; the table's variables applied from n (name, value) pairs standing in for the environment
const char* relax_host_option_key(int i) { return i >= 0 && i < relax::host::kNumOptions ? relax::host::kOptions[i].key : nullptr; }
void* relax_host_options_new(void) { return new relax::GemmOptions(); }
void relax_host_options_free(void* o) { delete static_cast<relax::GemmOptions*>(o); }
int relax_host_option_set(void* o, const char* key, int value, char* err, int err_len) {
    std::string e;
    if (relax::host::option_set(*static_cast<relax::GemmOptions*>(o), key, value, e)) return 0;
    if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s", e.c_str());
    return -1;
}
int relax_host_option_get(const void* o, const char* key, int* value, char* err, int err_len) {
    std::string e;
    if (relax::host::option_get(*static_cast<const relax::GemmOptions*>(o), key, value, e)) return 0;
    if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s", e.c_str());
    return -1;
}
void relax_host_options_from_env(void* o, const char* const* names, const char* const* values, int n) {
    relax::host::options_from_env(*static_cast<relax::GemmOptions*>(o), [&](const char* name) -> const char* {
        for (int i = 0; i < n; ++i)
            if (std::strcmp(names[i], name) == 0) return values[i];
        return nullptr;
    });
}

}  // extern "C"
#endif  // RELAX_HOST_TEST_API
