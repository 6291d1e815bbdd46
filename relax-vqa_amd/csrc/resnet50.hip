// ResNet-50 (torchvision v1.5 layout) feature extractor on gfx950: one forward per fragment yields the
// 15 layer-stack taps' spatial means (13120-d) and the avgpool vector + stats (2051-d).
//
// Reference semantics (file:line in xinyiW915/ReLaX-VQA):
//   src/extractor/visualise_resnet.py:40-50      preprocess: PNG(BGR->RGB), ToTensor (/255), Normalize(mean,std)
//   src/extractor/visualise_resnet.py:21,83-106  resnet50, one hooked forward per tap
//   src/main_fragment_layerstack.py:91-99        tap list; 'resnet50.conv1' is the RAW conv output (before bn1)
//   src/main_fragment_layerstack.py:134-149      spatial mean per tap / avgpool + (mean,max,std)
// Layout: activations NHWC fp32 (channel = GEMM N axis, contiguous), weights [Cout][KH*KW*Cin] with
// eval-mode BatchNorm folded in (scale into the weights, shift as bias); bn1 stays separate because
// the conv1 tap is taken before it.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "relax_internal.h"
#include "host_logic.h"

namespace relax {

int launch_gap_ws(relax_handle* h, const float* x, float* out, int Nimg, int HW, int C, int64_t out_stride,
                  float* partial_ws, hipStream_t s);

static const int kTapChannels[RELAX_RN50_NUM_TAPS] = {64, 256, 256, 256, 512, 512, 512, 512,
                                                      1024, 1024, 1024, 1024, 2048, 2048, 2048};

// ---- kernels ---------------------------------------------------------------------------------------
// uint8 BGR [N,Hc,Wc,3] -> fp32 NHWC4 RGB0, ((x/255) - mean) / std   (ToTensor + Normalize)
__global__ __launch_bounds__(256) void rn_preprocess(const uint8_t* __restrict__ frag, float* __restrict__ x,
                                                     int64_t npix) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const uint8_t* p = frag + i * 3;
    const float b = (float)p[0] / 255.0f, g = (float)p[1] / 255.0f, r = (float)p[2] / 255.0f;
    float4 o;
    o.x = (r - 0.485f) / 0.229f;
    o.y = (g - 0.456f) / 0.224f;
    o.z = (b - 0.406f) / 0.225f;
    o.w = 0.f;
    reinterpret_cast<float4*>(x)[i] = o;
}

// avgpool vector v[D] -> out[0:D] = v, out[D..D+2] = mean, max, population std  (D = 2048: ResNet-50's avgpool; 4096: VGG-16's fc2)
template <int D>
__global__ __launch_bounds__(256) void rn_pool_stats(const float* __restrict__ avg, int64_t avg_stride,
                                                     float* __restrict__ out, int64_t out_stride) {
    __shared__ float red[256];
    __shared__ float s_mean;
    const int n = blockIdx.x, t = threadIdx.x;
    const float* v = avg + (int64_t)n * avg_stride;
    float* o = out + (int64_t)n * out_stride;
    float vals[D / 256];
    float s = 0.f, m = -INFINITY;
#pragma unroll
    for (int j = 0; j < D / 256; ++j) {
        vals[j] = v[t + 256 * j];
        o[t + 256 * j] = vals[j];
        s += vals[j];
        m = fmaxf(m, vals[j]);
    }
    red[t] = s;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    if (t == 0) s_mean = red[0] / (float)D;
    __syncthreads();
    const float mean = s_mean;
    __syncthreads();
    red[t] = m;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (t < w) red[t] = fmaxf(red[t], red[t + w]);
        __syncthreads();
    }
    const float mx = red[0];
    __syncthreads();
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < D / 256; ++j) q += (vals[j] - mean) * (vals[j] - mean);
    red[t] = q;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    if (t == 0) {
        o[D] = mean;
        o[D + 1] = mx;
        o[D + 2] = sqrtf(red[0] / (float)D);
    }
}

int launch_pool_stats(relax_handle* h, const float* v, int64_t v_stride, float* out, int64_t out_stride, int n, int dim, hipStream_t s) {
    RELAX_REQUIRE(h, n > 0 && (dim == 2048 || dim == 4096), "pool_stats: n=%d dim=%d", n, dim);
    if (dim == 2048) hipLaunchKernelGGL(rn_pool_stats<2048>, dim3(n), dim3(256), 0, s, v, v_stride, out, out_stride);
    else hipLaunchKernelGGL(rn_pool_stats<4096>, dim3(n), dim3(256), 0, s, v, v_stride, out, out_stride);
    RELAX_HIP_CHECK(h, hipGetLastError());
    return RELAX_OK;
}

// ---- weights ---------------------------------------------------------------------------------------
// (key matching, BatchNorm folding and the OIHW -> [Cout][K] packing are host_logic.cpp: pure C++, sanitizer-tested on the CPU)
static constexpr float kBnEps = 1e-5f;

// conv (OIHW) [+ BN] -> device [Cout][Kpad] (+ bias).  cin_pad >= cin (conv1: 3 -> 4).
static int make_conv(relax_handle* h, const host::StateDict& sd, const std::string& conv, const std::string& bn, int cout,
                     int cin, int cin_pad, int k, int stride, int pad, ConvW* out, DeviceOwner& mem,
                     std::vector<float>* shift_out = nullptr) {
    std::string err;
    const float* w = sd.get(conv + ".weight", (int64_t)cout * cin * k * k, err);
    std::vector<float> scale(cout, 1.f), shift(cout, 0.f);
    RELAX_REQUIRE(h, w && (bn.empty() || host::read_bn(sd, bn, cout, kBnEps, scale.data(), shift.data(), err)), "%s", err.c_str());
    const int kpad = host::conv_kpad(k, cin_pad);
    std::vector<float> packed((size_t)cout * kpad);
    host::pack_conv_oihw(w, scale.data(), cout, cin, cin_pad, k, kpad, packed.data());
    out->Cin = cin_pad; out->Cout = cout; out->KH = k; out->KW = k; out->stride = stride; out->pad = pad;
    out->Kpad = kpad;
    // Hoelder constants of the folded convolution: |out[n]| <= l1max * max |in| + bmax  (per-image scales of the f16x2 layers, gemm_h2.hip)
    host::conv_hoelder(packed.data(), bn.empty() ? nullptr : shift.data(), cout, kpad, &out->l1max, &out->bmax);
    RELAX_TRY(mem.upload(h, packed.data(), packed.size(), &out->w));
    if (!bn.empty()) RELAX_TRY(mem.upload(h, shift.data(), shift.size(), &out->bias));
    else out->bias = nullptr;
    if (shift_out) *shift_out = shift;
    return RELAX_OK;
}

void free_resnet(relax_handle* h) {
    h->rn.mem.release();
    h->rn = ResNet50W();
}

// floats per image of the activation arena (see relax_resnet50_features): host_logic.cpp's rn_canvas_geometry, by the canvas - at 224 x 224
// x0 = 224*224*4, big = 112*112*64 (== 56*56*256), t1 = 56*56*128, t2 = 56*56*64, gap_ws = 196*256, block_max = 256
static constexpr size_t kAvg = host::kRnAvgFloats;
static constexpr size_t kImgSlots = host::kRnImgSlots;   // per-image tables of the f16x2 blocks: slot t = {maximum, scale, 1 / scale} x images

size_t resnet_arena_bytes(int n, int Hc, int Wc, int flags) {
    host::RnCanvasGeometry g;
    std::string err;
    if (!host::rn_canvas_geometry(Hc, Wc, flags, &g, err)) return 0;
    return sizeof(float) * (size_t)(g.floats_f32 > g.floats_x6 ? g.floats_f32 : g.floats_x6) * (size_t)n;
}

// RELAX_RN_FORCE_ANY_FORMS=1 in the environment (read once): a canvas set under RELAX_RN_CANVAS_ANY runs the any-size stem and max-pool even where the
// default rule takes it.  For tools/resnet_anysize_bench.py, which times the two forms of each on one canvas; not an option of the library.
static bool force_any_forms() {
    static const bool on = [] { const char* v = std::getenv("RELAX_RN_FORCE_ANY_FORMS"); return v && std::atoi(v) != 0; }();
    return on;
}

// the loader built what the plan's form of this block reads (both go by the predicates of host_logic.h)
static bool has_weights(const Bottleneck& k, const host::RnBlockPlan& q) {
    if (q.c1_h2 && !k.c1.w_h2) return false;
    switch (q.form) {
        case host::kRnFormH2: return k.c1.w_h2 && k.c2.w_h2 && k.c3.w_h2 && (!k.has_down || k.down.w_h2);
        case host::kRnFormB2BX2: return k.c2.w_h2 && k.c3d_w_h2p;
        case host::kRnFormB2BDown: return k.c2.w_h2 && k.c3.w_h2p && k.down.w_h2;
        case host::kRnFormB2B: return k.c2.w_h2 && k.c3.w_h2p;
        default: return (q.form == host::kRnFormX6 || k.c2.w_h2) && (!k.has_down || k.c3d_w_sp3);
    }
}

static int run_conv(relax_handle* h, const ConvW& c, const float* in, int Nimg, int H, int W, const float* residual,
                    float* out, int act, hipStream_t s, double flops = 0) {
    return launch_conv(h, conv_f32(c, in, Nimg, H, W, residual, out, act, flops), s);
}

// ---- derived weights --------------------------------------------------------------------------------------
// dst [rows][Ka + Kb] = [a | b] rows side by side
static int concat_rows(relax_handle* h, float* dst, const float* a, int Ka, const float* b, int Kb, int rows) {
    const size_t ld = sizeof(float) * (Ka + Kb);
    RELAX_HIP_CHECK(h, hipMemcpy2D(dst, ld, a, sizeof(float) * Ka, sizeof(float) * Ka, rows, hipMemcpyDeviceToDevice));
    RELAX_HIP_CHECK(h, hipMemcpy2D(dst + Ka, ld, b, sizeof(float) * Kb, sizeof(float) * Kb, rows, hipMemcpyDeviceToDevice));
    return RELAX_OK;
}

// the end of a conversion through staging rows: it is through (after a failed step too) before they are freed
static int built(relax_handle* h, int rc, const char* what) {
    if (hipDeviceSynchronize() != hipSuccess && rc == RELAX_OK) {
        set_error(h, "resnet50: building %s failed", what);
        rc = RELAX_ERR_HIP;
    }
    return rc;
}

// everything relax_load_resnet50 puts on the device; the caller frees it all if this fails
static int load_resnet(relax_handle* h, const host::StateDict& sd) {
    ResNet50W& rn = h->rn;
    RELAX_TRY(make_conv(h, sd, "conv1", "", 64, 3, 4, 7, 2, 3, &rn.conv1, rn.mem));
    {
        std::vector<float> sc(64), sh(64);
        std::string err;
        RELAX_REQUIRE(h, host::read_bn(sd, "bn1", 64, kBnEps, sc.data(), sh.data(), err), "%s", err.c_str());
        RELAX_TRY(rn.mem.upload(h, sc.data(), 64, &rn.bn1_scale));
        RELAX_TRY(rn.mem.upload(h, sh.data(), 64, &rn.bn1_shift));
    }
    const host::RnBlockGeom* geom = host::rn_geometry();
    for (int b = 0; b < host::kRnBlocks; ++b) {
        const host::RnBlockGeom& k = geom[b];
        Bottleneck blk;
        const std::string p = "layer" + std::to_string(k.layer) + "." + std::to_string(k.index);
        std::vector<float> shift3, shiftd;
        RELAX_TRY(make_conv(h, sd, p + ".conv1", p + ".bn1", k.width, k.cin, k.cin, 1, 1, 0, &blk.c1, rn.mem));
        RELAX_TRY(make_conv(h, sd, p + ".conv2", p + ".bn2", k.width, k.width, k.width, 3, k.stride, 1, &blk.c2, rn.mem));
        RELAX_TRY(make_conv(h, sd, p + ".conv3", p + ".bn3", k.cout, k.width, k.width, 1, 1, 0, &blk.c3, rn.mem, &shift3));
        blk.has_down = k.has_down;
        if (blk.has_down) {
            RELAX_TRY(make_conv(h, sd, p + ".downsample.0", p + ".downsample.1", k.cout, k.cin, k.cin, 1, k.stride, 0, &blk.down, rn.mem, &shiftd));
            for (size_t o = 0; o < shift3.size(); ++o) shift3[o] += shiftd[o];   // bias of the fused conv3 + downsample contraction
            RELAX_TRY(rn.mem.upload(h, shift3.data(), shift3.size(), &blk.c3d_bias));
        }
        blk.tap = k.tap;
        rn.blocks.push_back(blk);
    }
    // split planes for the bf16x6 kernels (made on the device from the packed fp32 copies): conv1 in its own K layout ...
    RELAX_TRY(make_conv1_x6_weights(h, rn.conv1.w, rn.conv1.Kpad, &rn.conv1.w_sp3, rn.mem));
    RELAX_TRY(make_conv1_h2_weights(h, rn.conv1.w, rn.conv1.Kpad, &rn.conv1.w_h2, &rn.conv1.w_inv, rn.mem));
    for (int b = 0; b < host::kRnBlocks; ++b) {
        Bottleneck& blk = rn.blocks[b];
        const host::RnBlockGeom& k = geom[b];
        const bool late = !host::rn_early(k);
        // ... every other convolution as [Cout][K] rows
        // ... the convolutions of layer3 / layer4 (256 / 512-wide, every Cout a multiple of 256, every Cin of 32) also as two fp16 planes with one
        // power-of-two scale per output row (gemm_h2.hip; w_inv = the inverse scales, the epilogue's colscale), and of layer1 / layer2 the
        // convolutions whose f16x2 form the schedule can ask for (host_logic.h: the 3x3, conv1, the downsample launch of layer2[0])
        const std::pair<ConvW*, bool> convs[] = {{&blk.c1, late || host::rn_early_h2(k.cin, k.width)}, {&blk.c2, late || host::rn_early_h2(k.width, k.width)},
                                                 {&blk.c3, late}, {&blk.down, k.has_down && (late || host::rn_can_down_launch(k))}};
        for (const auto& [c, as_h2] : convs) {
            if (!c->w) continue;
            const int K = c->KH * c->KW * c->Cin;
            RELAX_REQUIRE(h, K == c->Kpad && c->Cin % 16 == 0, "resnet50: conv K=%d (padded %d) does not fit the split-plane layout", K, c->Kpad);
            RELAX_TRY(derive_sp3(h, rn.mem, c->w, c->Cout, K, &c->w_sp3, "resnet50 split-plane weights"));
            if (!as_h2) continue;
            RELAX_REQUIRE(h, !late || (c->Cin % 32 == 0 && c->Cout % 256 == 0), "resnet50: fp16-plane weights of block %d (Cin %d, Cout %d) could not be made",
                          b, c->Cin, c->Cout);
            RELAX_TRY(derive_h2_rows(h, rn.mem, c->w, c->Cout, K, &c->w_h2, &c->w_inv, "resnet50 fp16-plane weights"));
        }
        const int Co = blk.c3.Cout;
        // ... conv3 of a block that can run back to back once more as fp16 planes with the K axis in the order of that form ("rn_fuse":
        // gemm_x6.hip, B2B - the 3x3's transposed accumulator tile is the A operand)
        if (host::rn_can_b2b(k)) {
            const int K = blk.c3.Cin;
            const char* what = "the back-to-back conv3 weights";
            ScopedDev perm;
            if (!perm.alloc(h, (size_t)Co * K, what)) return RELAX_ERR_NOMEM;
            int rc = launch_b2b_permute_k(h, blk.c3.w, perm.p, Co, K, nullptr);
            if (rc == RELAX_OK) rc = derive_h2_rows(h, rn.mem, perm.p, Co, K, &blk.c3.w_h2p, &blk.c3.w_invp, what);
            RELAX_TRY(built(h, rc, what));
        }
        // ... for layer1[0] [conv3 (K permuted) | downsample (natural K)] rows of 128 as fp16 planes: its back-to-back form contracts conv3 and
        // the downsample convolution in one accumulator (gemm_x6.hip, B2B == 2)
        if (host::rn_can_b2b_x2(k)) {
            const char* what = "the two-source back-to-back weights";
            ScopedDev perm, cat;
            if (!perm.alloc(h, (size_t)Co * 64, what) || !cat.alloc(h, (size_t)Co * 128, what)) return RELAX_ERR_NOMEM;
            int rc = built(h, launch_b2b_permute_k(h, blk.c3.w, perm.p, Co, 64, nullptr), what);
            if (rc == RELAX_OK) rc = concat_rows(h, cat.p, perm.p, 64, blk.down.w, 64, Co);
            if (rc == RELAX_OK) rc = derive_h2_rows(h, rn.mem, cat.p, Co, 128, &blk.c3d_w_h2p, &blk.c3d_w_invp, what);
            RELAX_TRY(built(h, rc, what));
        }
        // ... and, for the four blocks with a downsample branch, [conv3 | downsample] rows side by side as split planes
        if (blk.has_down) {
            const int K1 = blk.c3.Cin, K2 = blk.down.Cin;
            const char* what = "the fused conv3 + downsample weights";
            ScopedDev cat;
            if (!cat.alloc(h, (size_t)Co * (K1 + K2), what)) return RELAX_ERR_NOMEM;
            int rc = concat_rows(h, cat.p, blk.c3.w, K1, blk.down.w, K2, Co);
            if (rc == RELAX_OK) rc = derive_sp3(h, rn.mem, cat.p, Co, K1 + K2, &blk.c3d_w_sp3, what);
            RELAX_TRY(built(h, rc, what));
        }
    }
    if (hipDeviceSynchronize() != hipSuccess) {
        set_error(h, "resnet50: weight conversion failed");
        return RELAX_ERR_HIP;
    }
    return RELAX_OK;
}

}  // namespace relax

using namespace relax;

extern "C" {

int relax_load_resnet50(relax_handle* h, const float* const* tensors, const char* const* names,
                        const int64_t* numels, int n) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, tensors && names && numels && n > 0, "relax_load_resnet50: bad arguments");
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    free_resnet(h);
    host::StateDict sd;
    for (int i = 0; i < n; ++i) sd.add(names[i], tensors[i], numels[i]);
    const int rc = load_resnet(h, sd);
    if (rc == RELAX_OK) h->rn.loaded = true;
    else free_resnet(h);   // a failed load leaves nothing behind
    return rc;
}

int relax_resnet50_canvas_geometry(int Hc, int Wc, int* tap_hw, int64_t* arena_bytes_per_image) {
    return relax_resnet50_canvas_geometry_ex(Hc, Wc, 0, tap_hw, arena_bytes_per_image);
}

int relax_resnet50_canvas_geometry_ex(int Hc, int Wc, int flags, int* tap_hw, int64_t* arena_bytes_per_image) {
    host::RnCanvasGeometry g;
    std::string err;
    if (!host::rn_canvas_geometry(Hc, Wc, flags, &g, err)) {
        set_error(nullptr, "%s", err.c_str());   // (no handle: relax_last_error(NULL), this thread's)
        return RELAX_ERR_INVALID;
    }
    if (tap_hw) std::memcpy(tap_hw, g.tap_hw, sizeof(g.tap_hw));
    if (arena_bytes_per_image) *arena_bytes_per_image = (int64_t)resnet_arena_bytes(1, Hc, Wc, flags);
    return RELAX_OK;
}

// validation and two integers: no launch, no allocation, no synchronisation (the arena grows in the forward)
int relax_resnet50_set_canvas(relax_handle* h, int Hc, int Wc) { return relax_resnet50_set_canvas_ex(h, Hc, Wc, 0); }

int relax_resnet50_set_canvas_ex(relax_handle* h, int Hc, int Wc, int flags) {
    if (!h) return RELAX_ERR_INVALID;
    host::RnCanvasGeometry g;
    std::string err;
    RELAX_REQUIRE(h, host::rn_canvas_geometry(Hc, Wc, flags, &g, err), "%s", err.c_str());
    h->rn.canvas_h = Hc;
    h->rn.canvas_w = Wc;
    h->rn.canvas_flags = flags;
    return RELAX_OK;
}

int relax_resnet50_get_canvas(relax_handle* h, int* Hc, int* Wc) {
    if (!h) return RELAX_ERR_INVALID;
    if (Hc) *Hc = h->rn.canvas_h;
    if (Wc) *Wc = h->rn.canvas_w;
    return RELAX_OK;
}

// One forward over N images.  Images [0, n_ls) get layer-stack rows (n_ls = 0: none), images [pool_from, N) get pool rows
// (pool == nullptr: none); taps_nchw (all N images) as in relax_resnet50_features.
static int resnet_forward(relax_handle* h, const uint8_t* frags, int N, int n_ls, int pool_from, float* layer_stack, float* pool,
                          float* const* taps_nchw, hipStream_t s) {
    // the canvas is read here, once: a captured graph keeps the canvas it was captured with
    const int Hc = h->rn.canvas_h, Wc = h->rn.canvas_w;
    host::RnCanvas cv;
    cv.Hc = Hc; cv.Wc = Wc; cv.flags = h->rn.canvas_flags;
    cv.force_any = (cv.flags & host::kRnCanvasAny) && force_any_forms();
    host::RnCanvasGeometry geo;
    host::RnStemPlan stem;   // which stem and max-pool kernels take this canvas: the any-size forms only where the default rule refuses it
    {
        std::string geo_err;
        RELAX_REQUIRE(h, host::rn_canvas_geometry(Hc, Wc, cv.flags, &geo, geo_err) && host::rn_stem_plan(cv, &stem, geo_err), "%s", geo_err.c_str());
    }
    const size_t kX0 = (size_t)geo.x0, kBig = (size_t)geo.big, kT1 = (size_t)geo.t1, kT2 = (size_t)geo.t2, kGapWs = (size_t)geo.gap_ws;
    const int H0 = geo.tap_hw[0][0], W0 = geo.tap_hw[0][1];       // the stem's output (112 x 112)
    const int H1 = geo.tap_hw[1][0], W1 = geo.tap_hw[1][1];       // the max-pool's (56 x 56)
    const int HWlast = geo.tap_hw[RELAX_RN50_NUM_TAPS - 1][0] * geo.tap_hw[RELAX_RN50_NUM_TAPS - 1][1];   // layer4's map (49 positions)
    RELAX_TRY(ensure_buf(h, h->arena, resnet_arena_bytes(N, Hc, Wc, cv.flags)));
    float* base = static_cast<float*>(h->arena.p);
    const size_t n = (size_t)N;
    float* X0 = base;
    float* bufA = X0 + kX0 * n;
    float* bufB = bufA + kBig * n;
    float* bufD = bufB + kBig * n;
    float* T1 = bufD + kBig * n;
    float* T2 = T1 + kT1 * n;
    float* gapws = T2 + kT2 * n;
    float* avg = gapws + kGapWs * n;
    const ResNet50W& rn = h->rn;
    if (n_ls == 0) layer_stack = nullptr;
    const int n_pool = pool ? N - pool_from : 0;
    // the pool vector of an image that is also in the layer stack is the last 2048 columns of its layer-stack row
    const bool pool_from_stack = pool && layer_stack && pool_from == 0 && n_ls == N;

    auto tap_offset = [](int tap) {
        int off = 0;
        for (int t = 0; t < tap; ++t) off += kTapChannels[t];
        return off;
    };
    auto pool_tail = [&](const float* last32, float* avg_ws, float* gap_scratch) -> int {   // last32: fp32 [N,HWlast,2048] of the last block
        if (!pool) return RELAX_OK;
        const float* avg_src;
        int64_t avg_stride;
        if (pool_from_stack) {      // (layer_stack is non-null here; no pointer arithmetic on it otherwise)
            avg_src = layer_stack + (RELAX_RN50_LAYER_STACK_DIM - 2048);
            avg_stride = RELAX_RN50_LAYER_STACK_DIM;
        } else {
            RELAX_TRY(launch_gap_ws(h, last32 + (size_t)pool_from * HWlast * 2048, avg_ws, n_pool, HWlast, 2048, 2048, gap_scratch, s));
            avg_src = avg_ws;
            avg_stride = 2048;
        }
        return launch_pool_stats(h, avg_src, avg_stride, pool, RELAX_RN50_POOL_DIM, n_pool, 2048, s);
    };

    if (h->gemm.precision >= 2) {   // (3 = f16x2: layer3 / layer4 and the 3x3 convolutions of layer1 / layer2 on fp16 planes - "rn_h2", "rn_h2_early" - the rest bf16x6)
        // which launches run and in which form every tensor travels is host_logic.cpp's rn_plan (CPU-tested); here are the buffers and the launches
        const host::RnOptions opt{h->gemm.precision, h->gemm.rn_h2, h->gemm.rn_h2_early, h->gemm.rn_fuse, h->gemm.rn_c1_h2, h->gemm.fp32_rows};
        host::RnRequest rq{N, n_ls, pool_from, pool != nullptr, 0u};
        for (int t = 0; taps_nchw && t < RELAX_RN50_NUM_TAPS; ++t) rq.taps |= taps_nchw[t] ? 1u << t : 0u;
        host::RnPlan plan;
        std::string plan_err;
        RELAX_REQUIRE(h, rn.blocks.size() == (size_t)host::kRnBlocks && host::rn_plan(opt, rq, cv, (int)kImgSlots, &plan, plan_err), "%s",
                      plan_err.empty() ? "resnet50: not the 16 bottlenecks of the schedule" : plan_err.c_str());
        // bf16x6.  conv1 7x7/2 (raw) straight from the uint8 fragments (conv1_x6.hip: preprocess, im2col, split and contraction in one
        // kernel, the 16-pixel sums of the tap's spatial mean formed in its epilogue); from the max-pool on, every convolution input
        // travels as split planes written by its producer
        float* gap0 = T2 + kT2 * n;   // = the fp32 carving's gapws: free until the blocks carve the arena anew below
        RELAX_REQUIRE(h, !plan.conv1_h2 || rn.conv1.w_h2, "resnet50: the stem's fp16-plane weights are missing");
        const bool stem_mean = layer_stack && stem.stem_fused_mean;
        if (stem.stem_form == host::kRnStemAny)
            RELAX_TRY(launch_conv1_x6_any(h, frags, plan.conv1_h2 ? rn.conv1.w_h2 : rn.conv1.w_sp3, bufA, stem_mean ? gap0 : nullptr, N, Hc, Wc, s,
                                          plan.conv1_h2 ? rn.conv1.w_inv : nullptr));
        else
            RELAX_TRY(launch_conv1_x6(h, frags, plan.conv1_h2 ? rn.conv1.w_h2 : rn.conv1.w_sp3, bufA, stem_mean ? gap0 : nullptr, N, Hc, Wc, s,
                                      plan.conv1_h2 ? rn.conv1.w_inv : nullptr));
        if (stem_mean) RELAX_TRY(launch_gap_groups_finish(h, gap0, layer_stack, n_ls, H0 * W0, 64, RELAX_RN50_LAYER_STACK_DIM, s));
        else if (layer_stack) RELAX_TRY(launch_gap_ws(h, bufA, layer_stack, n_ls, H0 * W0, 64, RELAX_RN50_LAYER_STACK_DIM, gap0, s));   // (the raw output's mean, as the later taps')
        if (taps_nchw && taps_nchw[0]) RELAX_TRY(launch_nhwc_to_nchw(h, bufA, taps_nchw[0], N, H0 * W0, 64, s));
        float* f32a = bufB;                                   // block outputs as fp32, where something needs them (ping-pong with f32b)
        float* f32b = bufD;
        char* spa = reinterpret_cast<char*>(T1);              // carve the rest of the arena anew
        char* spb = spa + sizeof(float) * (kBig * 3 / 2) * n;
        char* T1s = spb + sizeof(float) * (kBig * 3 / 2) * n;
        char* T2s = T1s + sizeof(float) * (kT1 * 3 / 2) * n;
        gapws = reinterpret_cast<float*>(T2s + sizeof(float) * (kT2 * 3 / 2) * n);
        float* avg6 = gapws + kGapWs * n;
        // per-image tables {maximum, scale, 1 / scale} of the f16x2 launches, one slot per tensor (the plan's s_* fields)
        float* imgtab = avg6 + kAvg * n;
        auto slot_amax = [&](int t) { return reinterpret_cast<unsigned*>(imgtab + (size_t)(3 * t) * n); };
        auto slot_scale = [&](int t) { return imgtab + (size_t)(3 * t + 1) * n; };
        auto slot_inv = [&](int t) { return imgtab + (size_t)(3 * t + 2) * n; };
        // slot t's scale and inverse from Hoelder's bound  la max(a) + lb max(b) + max(r) + c  over measured maxima (-1: no such term)
        auto scales = [&](int t, int a, float la, int b, float lb, int r, float c) {
            return launch_h2_image_scales(h, slot_amax(a), la, b >= 0 ? slot_amax(b) : nullptr, lb, r >= 0 ? slot_amax(r) : nullptr, c, slot_scale(t),
                                          slot_inv(t), N, s);
        };
        auto conv_h2 = [&](const ConvW& c, const void* in, int Hin, int Win, int slot_in, GemmDescH2 g, int slot_out, int act) {
            g = relax::conv_h2(c, in, N, Hin, Win, act, g);
            g.img_in_inv = slot_inv(slot_in);
            if (g.out_h2) { g.img_out_scale = slot_scale(slot_out); g.amax_out = slot_amax(slot_out); }
            return launch_gemm_h2(h, g, s);
        };
        if (plan.n_slots) RELAX_HIP_CHECK(h, fill_async(imgtab, 0, sizeof(float) * 3 * kImgSlots * n, s));
        unsigned* blockmax = reinterpret_cast<unsigned*>(imgtab + 3 * kImgSlots * n);
        if (stem.pool_form == host::kRnPoolAny)   // (block maxima with a ragged last block per image: geo.block_max words per image hold them)
            RELAX_TRY(launch_bn_relu_maxpool_any(h, bufA, rn.bn1_scale, rn.bn1_shift, plan.pool_f32 ? bufD : nullptr, plan.pool_f32 ? nullptr : spa, N, H0, W0, 64, s,
                                                 plan.s_stem >= 0 ? slot_amax(plan.s_stem) : nullptr, blockmax));
        else if (plan.pool_f32)
            RELAX_TRY(launch_bn_relu_maxpool_f32(h, bufA, rn.bn1_scale, rn.bn1_shift, bufD, N, H0, W0, 64, s, slot_amax(plan.s_stem), blockmax));
        else
            RELAX_TRY(launch_bn_relu_maxpool_sp3(h, bufA, rn.bn1_scale, rn.bn1_shift, spa, N, H0, W0, 64, s,
                                                 plan.s_stem >= 0 ? slot_amax(plan.s_stem) : nullptr, blockmax));
        const float* cur32 = plan.pool_f32 ? bufD : nullptr;   // (f32b: block 0 writes f32a, block 1 - which overwrites f32b - runs when block 0 is through)
        char* cursp = spa;       // the block input's planes; a stride-2 sample the previous block left (in_sample) lies in othersp
        char* othersp = spb;
        float* out32 = f32a;
        int H = H1, W = W1;
        for (size_t b = 0; b < rn.blocks.size(); ++b) {
            const Bottleneck& blk = rn.blocks[b];
            const host::RnBlockPlan& q = plan.blk[b];
            const int Ho = conv_out(H, blk.c2.KH, blk.c2.stride, blk.c2.pad), Wo = conv_out(W, blk.c2.KW, blk.c2.stride, blk.c2.pad);
            const int HWo = Ho * Wo, Cout = blk.c3.Cout;
            const bool b2b = q.form == host::kRnFormB2B || q.form == host::kRnFormB2BX2 || q.form == host::kRnFormB2BDown;
            float* y32 = q.need32 ? out32 : nullptr;
            float* gap = q.fuse_mean ? gapws : nullptr;
            RELAX_REQUIRE(h, has_weights(blk, q), "resnet50: block %zu lacks the derived weights of launch form %d", b, q.form);
            if (q.form == host::kRnFormH2) {
                // ---- an f16x2 block (gemm_h2.hip): cursp = the block input's planes (slot s_in)
                // conv1 1x1 + ReLU
                RELAX_TRY(scales(q.s_t1, q.s_in, blk.c1.l1max, -1, 0.f, -1, blk.c1.bmax));
                { GemmDescH2 g{}; g.out_h2 = T1s; RELAX_TRY(conv_h2(blk.c1, cursp, H, W, q.s_in, g, q.s_t1, 1)); }
                // conv2 3x3 (stride) + ReLU
                RELAX_TRY(scales(q.s_t2, q.s_t1, blk.c2.l1max, -1, 0.f, -1, blk.c2.bmax));
                { GemmDescH2 g{}; g.out_h2 = T2s; RELAX_TRY(conv_h2(blk.c2, T1s, H, W, q.s_t1, g, q.s_t2, 1)); }
                // conv3 1x1 + identity + ReLU: the identity is the block input (its planes) or the downsample convolution of it (fp32, no
                // activation; bounded by its own Hoelder term)
                GemmDescH2 g3{};
                if (blk.has_down) {
                    GemmDescH2 gd{};
                    gd.out = bufA;
                    RELAX_TRY(conv_h2(blk.down, cursp, H, W, q.s_in, gd, -1, 0));
                    g3.residual = bufA;
                    RELAX_TRY(scales(q.s_out, q.s_t2, blk.c3.l1max, q.s_in, blk.down.l1max, -1, blk.c3.bmax + blk.down.bmax));
                } else {
                    g3.residual_h2 = cursp; g3.img_res_inv = slot_inv(q.s_in);
                    RELAX_TRY(scales(q.s_out, q.s_t2, blk.c3.l1max, -1, 0.f, q.s_in, blk.c3.bmax));
                }
                g3.out = y32; g3.out_rows = q.rows32;
                g3.out_h2 = q.out_form == host::kRnH2 ? othersp : nullptr;
                g3.gap_groups = gap; g3.gap_rows = n_ls * HWo;
                g3.no_split = q.no_split;
                RELAX_TRY(conv_h2(blk.c3, T2s, Ho, Wo, q.s_t2, g3, q.s_out, 1));
            } else {
                // ---- conv1 1x1 + ReLU, from fp32 rows (split in the K loop) or planes
                const bool in_f32 = q.in_form == host::kRnF32;
                ConvDescX6 d = conv_x6(blk.c1, in_f32 ? static_cast<const void*>(cur32) : cursp, N, H, W);
                d.in_f32 = in_f32;
                if (q.c1_h2) {
                    // f16x2: the rows are split into fp16 planes in the K loop, with the image's scale from the MEASURED maximum of the block input
                    RELAX_TRY(scales(q.s_c1, q.s_in_max, 1.f, -1, 0.f, -1, 0.f));
                    d.w = blk.c1.w_h2; d.colscale = blk.c1.w_inv; d.img_in_scale = slot_scale(q.s_c1); d.img_in_inv = slot_inv(q.s_c1);
                }
                if (q.s_t1 >= 0) {   // fp16 planes for the f16x2 conv2, scaled by the image's bound
                    RELAX_TRY(scales(q.s_t1, q.s_in_max, blk.c1.l1max, -1, 0.f, -1, blk.c1.bmax));
                    d.out_h2 = T1s; d.img_out_scale = slot_scale(q.s_t1);
                    if (q.s_t1m >= 0) d.amax_out = slot_amax(q.s_t1m);
                } else {
                    d.out_sp3 = T1s;
                }
                RELAX_TRY(launch_conv_x6(h, d, s));
                // ---- conv2 3x3 (stride) + ReLU; back to back, conv3 in the same launch
                ConvDescX6 d2 = conv_x6(blk.c2, T1s, N, H, W);
                if (q.s_t1 >= 0) { d2.in_h2 = 1; d2.w = blk.c2.w_h2; d2.colscale = blk.c2.w_inv; d2.img_in_inv = slot_inv(q.s_t1); }
                // ---- conv3 1x1 + identity + ReLU.  Its output: fp32 rows where the plan wants them, and bf16 planes, or - the hand-over block - fp16
                // planes with a per-image scale, or fp32 rows only plus the planes of the stride-2 sample the next block's downsample branch reads
                ConvDescX6 d3 = conv_x6(blk.c3, T2s, N, Ho, Wo);
                ConvDescX6& y = b2b ? d2 : d3;      // the launch that writes the block output
                int s_planes = q.handover ? q.s_out : q.s_dr_out;   // scale of the fp16 planes the block output leaves as, if any
                if (b2b) {
                    d2.w3 = blk.c3.w_h2p; d2.colscale3 = blk.c3.w_invp; d2.bias3 = blk.c3.bias; d2.Cout3 = Cout;
                    d2.residual = cur32;
                    if (q.form == host::kRnFormB2BDown) {
                        // the downsample branch first: fp32 [N*Ho*Wo][Cout] into bufA (the stem's raw output: dead since the max-pool), on gemm_h3's
                        // 1x1 form from the compact fp16 planes of the input's stride-2 sample the previous block left (its per-image scale: s_dr_in)
                        ConvW down1 = blk.down;
                        down1.stride = 1;
                        GemmDescH2 g{};
                        g.out = bufA;
                        RELAX_TRY(conv_h2(down1, othersp, Ho, Wo, q.s_dr_in, g, -1, 0));
                        d2.residual = bufA;
                    }
                    if (q.form == host::kRnFormB2BX2) { d2.w3 = blk.c3d_w_h2p; d2.colscale3 = blk.c3d_w_invp; d2.bias3 = blk.c3d_bias; d2.residual = nullptr; d2.x2 = cur32; }
                    // fp16 planes with a per-image scale from a bound.  Two launches: Hoelder on conv3 with the MEASURED maximum of conv2's
                    // output; back to back that tensor never exists, so it is bounded in turn from the measured maximum of conv1's output:
                    // |y| <= l1(c3) (l1(c2) max|t1| + b2) + b3 + max|x|  - one more L1-to-max ratio of looseness (2^5 - 2^7 of fp16's 19
                    // binades), still never compounding beyond this block
                    if (s_planes >= 0)
                        RELAX_TRY(scales(s_planes, q.s_t1m, blk.c3.l1max * blk.c2.l1max, -1, 0.f, q.s_in_max, blk.c3.l1max * blk.c2.bmax + blk.c3.bmax));
                    d2.sp3_sub = q.out_sample != host::kRnNoSample ? 2 : 1;
                } else {
                    if (q.handover) d2.amax_out = slot_amax(q.s_t2);
                    d2.out_sp3 = T2s;
                    RELAX_TRY(launch_conv_x6(h, d2, s));
                    d3.no_split = q.no_split;
                    if (blk.has_down) {
                        // conv3 and the downsample convolution in ONE contraction over K = [conv2 output | block input sampled with the
                        // block's stride]: no fp32 copy of the branch is written and read back (layer1.0: 6.6 GB per 1024 images)
                        d3.w = blk.c3d_w_sp3; d3.bias = blk.c3d_bias;
                        d3.in2 = cursp; d3.H2 = H; d3.W2 = W; d3.Cin2 = blk.down.Cin; d3.stride2 = blk.down.stride;
                        if (q.in_sample == host::kRnSampleSp3) { d3.in2 = othersp; d3.H2 = Ho; d3.W2 = Wo; d3.stride2 = 1; }   // (the previous block left the stride-2 sample only)
                    } else if (in_f32) {
                        d3.residual = cur32;
                    } else {
                        d3.residual_sp3 = cursp;
                    }
                    // (block 6 has no downsample branch and its input is fp32 rows; its output leaves as fp16 planes with the Hoelder scale of
                    // conv3 + identity; block 7 takes its identity from its downsample branch)
                    if (q.handover) RELAX_TRY(scales(s_planes, q.s_t2, blk.c3.l1max, -1, 0.f, q.s_in_max, blk.c3.bmax));
                }
                y.out = y32; y.out_rows = q.rows32;
                y.gap_groups = gap; y.gap_rows = n_ls * HWo;
                y.out_sp3 = (q.out_form == host::kRnSp3 || q.out_sample == host::kRnSampleSp3) ? othersp : nullptr;
                if (s_planes >= 0) { y.out_h2 = othersp; y.img_out_scale = slot_scale(s_planes); }
                y.amax_out = q.s_out >= 0 ? slot_amax(q.s_out) : nullptr;
                RELAX_TRY(launch_conv_x6(h, y, s));
            }
            // ---- the block is through: its output becomes the next block's input; the tap
            cur32 = y32;
            if (y32) out32 = out32 == f32a ? f32b : f32a;
            if (q.out_form != host::kRnF32) { char* t = cursp; cursp = othersp; othersp = t; }   // (fp32 rows: a stride-2 sample, if any, stays in othersp)
            H = Ho; W = Wo;
            const int off = q.want_mean ? tap_offset(blk.tap) : 0;
            if (q.fuse_mean)
                RELAX_TRY(launch_gap_groups_finish(h, gapws, layer_stack + off, n_ls, HWo, Cout, RELAX_RN50_LAYER_STACK_DIM, s));
            else if (q.want_mean)
                RELAX_TRY(launch_gap_ws(h, cur32, layer_stack + off, n_ls, HWo, Cout, RELAX_RN50_LAYER_STACK_DIM, gapws, s));
            if (q.want_export) RELAX_TRY(launch_nhwc_to_nchw(h, cur32, taps_nchw[blk.tap], N, HWo, Cout, s));
        }
        return pool_tail(cur32, avg6, gapws);
    }
    auto emit_tap = [&](int tap, const float* act) -> int {
        const int C = kTapChannels[tap], HW = geo.tap_hw[tap][0] * geo.tap_hw[tap][1];
        if (layer_stack)
            RELAX_TRY(launch_gap_ws(h, act, layer_stack + tap_offset(tap), n_ls, HW, C, RELAX_RN50_LAYER_STACK_DIM, gapws, s));
        if (taps_nchw && taps_nchw[tap]) RELAX_TRY(launch_nhwc_to_nchw(h, act, taps_nchw[tap], N, HW, C, s));
        return RELAX_OK;
    };
    const int64_t npix = (int64_t)N * Hc * Wc;
    hipLaunchKernelGGL(rn_preprocess, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, frags, X0, npix);
    RELAX_HIP_CHECK(h, hipGetLastError());
    // conv1 7x7/2 (raw), algorithmic FLOPs use the real 3 input channels
    RELAX_TRY(run_conv(h, rn.conv1, X0, N, Hc, Wc, nullptr, bufA, 0, s, 2.0 * N * (double)H0 * W0 * 64.0 * 147.0));
    RELAX_TRY(emit_tap(0, bufA));
    if (stem.pool_form == host::kRnPoolAny)
        RELAX_TRY(launch_bn_relu_maxpool_any(h, bufA, rn.bn1_scale, rn.bn1_shift, bufB, nullptr, N, H0, W0, 64, s, nullptr, nullptr));
    else
        RELAX_TRY(launch_bn_relu_maxpool(h, bufA, rn.bn1_scale, rn.bn1_shift, bufB, N, H0, W0, 64, s));
    float* cur = bufB;
    float* other = bufA;
    int H = H1, W = W1;
    for (const Bottleneck& blk : rn.blocks) {
        const int Ho = conv_out(H, blk.c2.KH, blk.c2.stride, blk.c2.pad), Wo = conv_out(W, blk.c2.KW, blk.c2.stride, blk.c2.pad);
        RELAX_TRY(run_conv(h, blk.c1, cur, N, H, W, nullptr, T1, 1, s));
        RELAX_TRY(run_conv(h, blk.c2, T1, N, H, W, nullptr, T2, 1, s));
        const float* identity = cur;
        if (blk.has_down) {
            RELAX_TRY(run_conv(h, blk.down, cur, N, H, W, nullptr, bufD, 0, s));
            identity = bufD;
        }
        RELAX_TRY(run_conv(h, blk.c3, T2, N, Ho, Wo, identity, other, 1, s));
        float* t = cur; cur = other; other = t;
        H = Ho; W = Wo;
        if (blk.tap >= 0) RELAX_TRY(emit_tap(blk.tap, cur));
    }
    return pool_tail(cur, avg, gapws);
}

int relax_resnet50_features(relax_handle* h, const uint8_t* frags, int N, float* layer_stack, float* pool,
                            float* const* taps_nchw, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, h->rn.loaded, "relax_resnet50_features: call relax_load_resnet50 first");
    RELAX_REQUIRE(h, frags && N > 0, "relax_resnet50_features: bad arguments");
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    return resnet_forward(h, frags, N, layer_stack ? N : 0, 0, layer_stack, pool, taps_nchw, static_cast<hipStream_t>(stream));
}

int relax_resnet50_clip_features(relax_handle* h, const uint8_t* frags, int N, int n_layer_stack, float* layer_stack, float* pool,
                                 relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, h->rn.loaded, "relax_resnet50_clip_features: call relax_load_resnet50 first");
    RELAX_REQUIRE(h, frags && N > 0 && n_layer_stack >= 0 && n_layer_stack <= N, "relax_resnet50_clip_features: bad arguments");
    RELAX_REQUIRE(h, (n_layer_stack == 0 || layer_stack) && (n_layer_stack == N || pool),
                  "relax_resnet50_clip_features: NULL output for a non-empty group of images");
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    return resnet_forward(h, frags, N, n_layer_stack, n_layer_stack, layer_stack, n_layer_stack < N ? pool : nullptr, nullptr,
                          static_cast<hipStream_t>(stream));
}

}  // extern "C"
