// VGG-16 (torchvision configuration D, no BatchNorm) feature extractor on gfx950: one forward per fragment yields the 13 convolution
// taps' spatial means (4224-d layer stack) and fc2 + stats (4099-d pool vector).
//
// Reference semantics (file:line in xinyiW915/ReLaX-VQA):
//   src/extractor/visualise_vgg.py:38-58          preprocess Resize/ToTensor/Normalize; one hooked forward per features[i]
//   src/extractor/visualise_vgg_layer.py:36-66    'fc1' = classifier[0], 'fc2' = classifier[3]
//   src/main_fragment_layerstack.py:101-108       tap list [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28] / 'fc2'
//   src/main_fragment_layerstack.py:124-160       spatial mean per tap / fc2 + (mean, max, std)
// torchvision builds VGG with ReLU(inplace=True) right behind every hooked module, so each hooked output is rectified in place before the
// hook's reference is read: every tap (and fc1 / fc2) is POST-ReLU.  Dropout is the identity in eval, AdaptiveAvgPool2d(7) the identity at 224^2.
//
// Layout: activations NHWC (channel contiguous), rows = pixels.  conv1_1 (3 -> 64, K = 27) is a streaming kernel of its own that reads the
// uint8 BGR fragments; the other 12 convolutions and both classifier layers run on the project's contraction kernels, with bias + ReLU fused:
//   "gemm_precision" 3  f16x2: gemm_x6<H2> for the 3x3s onto 64 / 128 channels, gemm_h3 (conv form) for 256 / 512 channels and the classifier
//                       layers (1x1 convolutions over 1x1 "images": per-image scales).  Per-image scales as in ResNet-50: a tensor's scale is
//                       fixed before it is written, from Hoelder's bound  l1max(W) * (measured max of the input) + bmax  of its producer; a
//                       max-pool output takes the measured maximum of the convolution in front of it (the pool does not raise it).
//   "gemm_precision" 2  bf16x6 everywhere (split planes written by the producer's epilogue).
//   "gemm_precision" 0  the exact-fp32 kernel on fp32 rows (1: bf16x3, opt-in).
// Images go through in chunks of at most kVggChunk (the 224^2 x 64 maps are 12.8 MB per image in fp32).
#include <cmath>

#include "relax_internal.h"
#include "host_logic.h"
#include "h2.h"
#include "sp3.h"

namespace relax {

static constexpr int kVggChunk = 32;            // images per pass through the network (workspace: vgg_arena_bytes(kVggChunk), ~1.7 GB)
static constexpr int kVggSlots = 24;            // per-image tables {maximum, scale, 1 / scale}: 13 convolutions + 5 pools + fc1 + fc2 = 20 used
static const int kVggHW[host::kVggConvs] = {224, 224, 112, 112, 56, 56, 56, 28, 28, 28, 14, 14, 14};
static const bool kVggPoolAfter[host::kVggConvs] = {false, true, false, true, false, false, true, false, false, true, false, false, true};

// floats per image of the arena
static constexpr size_t kMap = (size_t)224 * 224 * 64;          // the largest activation (conv1_x output)
static constexpr size_t kPlanes = kMap * 3 / 2;                 // ... as split planes (6 B per value; fp16 planes and fp32 take 4)
static constexpr size_t kGroups = (size_t)224 * 224 / 16 * 64;  // group sums of the fused spatial mean (largest: 16-row groups at 224^2, = 4-row at 56^2 x 256)
static constexpr size_t kFc = 4096;
static constexpr size_t kVggFloatsPerImage = kMap + 2 * kPlanes + kGroups + 2 * kFc + 3 * kVggSlots;

size_t vgg_arena_bytes(int n) {
    const size_t c = (size_t)(n < kVggChunk ? n : kVggChunk);
    return sizeof(float) * kVggFloatsPerImage * c;
}

// ---- kernels ---------------------------------------------------------------------------------------

// conv1_1: uint8 BGR [N,224,224,3] -> BGR->RGB, /255, (x - mean) / std -> 3x3 conv 3 -> 64 (pad 1) -> + bias -> ReLU.
// A block takes 512 consecutive pixels of one image (98 blocks per image); thread t: 16 consecutive pixels (t / 8) x 8 channels (t % 8).
// Writes any of: fp32 rows [M][64], fp16 planes [M][64*4 B] scaled by `h2_scale`, split planes [M][64*6 B]; the 16-row group sums of the
// tap's spatial mean [M/16][64]; the per-image maximum (atomicMax on the bits: the outputs are >= 0); img_scale / img_inv [N] = h2_scale, 1 / it.
constexpr int kC11Pix = 512;
constexpr int kC11Rows = 5;   // input rows a block touches: 512 pixels span at most 4 rows of 224, plus the halo above and below (<= 6; see below)
__global__ __launch_bounds__(256) void vgg_conv1_1(const uint8_t* __restrict__ frags, const float* __restrict__ w, const float* __restrict__ bias,
                                                   float* __restrict__ out, char* __restrict__ out_h2, float h2_scale, char* __restrict__ out_sp3,
                                                   float* __restrict__ gap, unsigned* __restrict__ amax, float* __restrict__ img_scale,
                                                   float* __restrict__ img_inv) {
    constexpr int HW = 224 * 224;
    __shared__ float4 s_in[kC11Rows + 1][226];       // normalised RGB0, columns -1 .. 224 (zero padding)
    __shared__ float4 s_w[8][27][2];                 // [channel group][k][8 channels]
    __shared__ unsigned s_max;
    const int n = blockIdx.y, t = threadIdx.x;
    const int p0 = blockIdx.x * kC11Pix;
    const int y0 = p0 / 224 - 1;                     // first staged input row (may be -1)
    const int y1 = (p0 + kC11Pix - 1) / 224 + 1;     // last (may be 224)
    const int rows = y1 - y0 + 1;                    // <= 6 (512 pixels touch at most 4 output rows)
    if (t == 0) s_max = 0u;
    for (int i = t; i < 64 * 27; i += 256) {         // w: [64][32], k = (dy*3 + dx)*3 + c
        const int o = i / 27, k = i % 27;
        reinterpret_cast<float*>(&s_w[o >> 3][k][0])[o & 7] = w[o * 32 + k];
    }
    const uint8_t* img = frags + (int64_t)n * HW * 3;
    for (int i = t; i < rows * 226; i += 256) {
        const int r = i / 226, xx = i % 226 - 1, y = y0 + r;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (y >= 0 && y < 224 && xx >= 0 && xx < 224) {
            const uint8_t* q = img + ((int64_t)y * 224 + xx) * 3;
            const float b = (float)q[0] / 255.0f, g = (float)q[1] / 255.0f, rr = (float)q[2] / 255.0f;
            v.x = (rr - 0.485f) / 0.229f;
            v.y = (g - 0.456f) / 0.224f;
            v.z = (b - 0.406f) / 0.225f;
        }
        s_in[r][xx + 1] = v;
    }
    __syncthreads();
    const int cg = t & 7, grp = t >> 3;
    float bsum[8], bias8[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) { bsum[o] = 0.f; bias8[o] = bias[cg * 8 + o]; }
    float mx = 0.f;
    for (int j = 0; j < 16; ++j) {
        const int p = p0 + grp * 16 + j;
        const int y = p / 224, x = p % 224;
        float acc[8];
#pragma unroll
        for (int o = 0; o < 8; ++o) acc[o] = 0.f;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const float4 v = s_in[y - 1 + dy - y0][x + dx];
                const float vc[3] = {v.x, v.y, v.z};
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int k = (dy * 3 + dx) * 3 + c;
                    const float4 wa = s_w[cg][k][0], wb = s_w[cg][k][1];
                    acc[0] = fmaf(vc[c], wa.x, acc[0]); acc[1] = fmaf(vc[c], wa.y, acc[1]);
                    acc[2] = fmaf(vc[c], wa.z, acc[2]); acc[3] = fmaf(vc[c], wa.w, acc[3]);
                    acc[4] = fmaf(vc[c], wb.x, acc[4]); acc[5] = fmaf(vc[c], wb.y, acc[5]);
                    acc[6] = fmaf(vc[c], wb.z, acc[6]); acc[7] = fmaf(vc[c], wb.w, acc[7]);
                }
            }
        }
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            acc[o] = fmaxf(acc[o] + bias8[o], 0.f);
            bsum[o] += acc[o];
            mx = fmaxf(mx, acc[o]);
        }
        const int64_t row = (int64_t)n * HW + p;
        const h2_f32x4 a = {acc[0], acc[1], acc[2], acc[3]}, b = {acc[4], acc[5], acc[6], acc[7]};
        if (out) {
            float4* d = reinterpret_cast<float4*>(out + row * 64 + cg * 8);
            d[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
            d[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
        }
        if (out_h2) store_h2_x8(out_h2 + row * 64 * 4, cg * 8, a, b, h2_scale);
        if (out_sp3) store_sp3_x8(out_sp3 + row * 64 * 6, cg * 8, a, b);
    }
    if (gap) {
        float4* d = reinterpret_cast<float4*>(gap + (((int64_t)n * HW + p0) / 16 + grp) * 64 + cg * 8);
        d[0] = make_float4(bsum[0], bsum[1], bsum[2], bsum[3]);
        d[1] = make_float4(bsum[4], bsum[5], bsum[6], bsum[7]);
    }
    if (amax) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        if ((t & 63) == 0) atomicMax(&s_max, __float_as_uint(mx));
        __syncthreads();
        if (t == 0) atomicMax(amax + n, s_max);
    }
    if (img_scale && blockIdx.x == 0 && t == 0) {
        img_scale[n] = h2_scale;
        img_inv[n] = 1.f / h2_scale;
    }
}

// 2x2 / stride-2 max-pool, NHWC fp32 [N][H][W][C] -> [N][H/2][W/2][C] as fp32 (OUT 0), fp16 planes scaled by img_scale[image] (OUT 1)
// or split planes (OUT 2).  One thread: one output pixel x 8 channels.
template <int OUT>
__global__ __launch_bounds__(256) void vgg_maxpool2x2(const float* __restrict__ x, void* __restrict__ y, const float* __restrict__ img_scale,
                                                      int n_img, int H, int W, int C) {
    const int Ho = H / 2, Wo = W / 2, cg8 = C / 8;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n_img * Ho * Wo * cg8) return;
    const int cg = (int)(i % cg8);
    const int64_t q = i / cg8;                        // output pixel
    const int ox = (int)(q % Wo), oy = (int)((q / Wo) % Ho), n = (int)(q / ((int64_t)Ho * Wo));
    const float* src = x + (((int64_t)n * H + 2 * oy) * W + 2 * ox) * C + cg * 8;
    float4 a = reinterpret_cast<const float4*>(src)[0], b = reinterpret_cast<const float4*>(src)[1];
    const int64_t offs[3] = {(int64_t)C, (int64_t)W * C, (int64_t)W * C + C};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float4 c0 = reinterpret_cast<const float4*>(src + offs[j])[0], c1 = reinterpret_cast<const float4*>(src + offs[j])[1];
        a.x = fmaxf(a.x, c0.x); a.y = fmaxf(a.y, c0.y); a.z = fmaxf(a.z, c0.z); a.w = fmaxf(a.w, c0.w);
        b.x = fmaxf(b.x, c1.x); b.y = fmaxf(b.y, c1.y); b.z = fmaxf(b.z, c1.z); b.w = fmaxf(b.w, c1.w);
    }
    if (OUT == 0) {
        float4* d = reinterpret_cast<float4*>(static_cast<float*>(y) + q * C + cg * 8);
        d[0] = a;
        d[1] = b;
    } else if (OUT == 1) {
        store_h2_x8(static_cast<char*>(y) + q * C * 4, cg * 8, (h2_f32x4){a.x, a.y, a.z, a.w}, (h2_f32x4){b.x, b.y, b.z, b.w}, img_scale[n]);
    } else {
        store_sp3_x8(static_cast<char*>(y) + q * C * 6, cg * 8, (sp3_f32x4){a.x, a.y, a.z, a.w}, (sp3_f32x4){b.x, b.y, b.z, b.w});
    }
}

// ---- weights ---------------------------------------------------------------------------------------
void free_vgg(relax_handle* h) {
    h->vgg.mem.release();
    h->vgg = VggW();
}

// packed fp32 [Cout][K] rows on the host -> device copies in the three formats (fp32, split planes, fp16 planes + inverse row scales),
// and the Hoelder constants |out[n]| <= l1max * max |in| + bmax
static int make_rows(relax_handle* h, const std::vector<float>& packed, const float* bias, int cout, int k, ConvW* c, DeviceOwner& mem, bool planes) {
    c->Cout = cout; c->Kpad = k;
    host::conv_hoelder(packed.data(), bias, cout, k, &c->l1max, &c->bmax);
    RELAX_TRY(mem.upload(h, packed.data(), packed.size(), &c->w));
    RELAX_TRY(mem.upload(h, bias, (size_t)cout, &c->bias));
    if (!planes) return RELAX_OK;
    RELAX_TRY(derive_sp3(h, mem, c->w, cout, k, &c->w_sp3, "vgg16 split-plane weights"));
    RELAX_TRY(derive_h2_rows(h, mem, c->w, cout, k, &c->w_h2, &c->w_inv, "vgg16 fp16-plane weights"));
    RELAX_HIP_CHECK(h, hipDeviceSynchronize());
    return RELAX_OK;
}

static int load_vgg(relax_handle* h, const host::StateDict& sd) {
    VggW& v = h->vgg;
    std::string err;
    if (!host::vgg16_check_keys(sd, err)) {
        set_error(h, "relax_load_vgg16: %s", err.c_str());
        return RELAX_ERR_INVALID;
    }
    for (int i = 0; i < host::kVggConvs; ++i) {
        const int cin = host::kVggConvCin[i], cout = host::kVggConvCout[i];
        const std::string p = "features." + std::to_string(host::kVggFeatureIndex[i]);
        const float* w = sd.get(p + ".weight", (int64_t)cout * cin * 9, err);
        const float* b = sd.get(p + ".bias", cout, err);
        const int kpad = host::conv_kpad(3, cin);
        std::vector<float> packed((size_t)cout * kpad);
        host::pack_conv_oihw(w, nullptr, cout, cin, cin, 3, kpad, packed.data());
        ConvW& c = v.conv[i];
        RELAX_TRY(make_rows(h, packed, b, cout, kpad, &c, v.mem, i > 0));
        c.Cin = cin; c.KH = 3; c.KW = 3; c.stride = 1; c.pad = 1;
    }
    {   // conv1_1 writes fp16 planes with one static scale: its input is bounded by the normalisation, |(x - mean) / std| <= max over the
        // channels of max(mean, 1 - mean) / std for x in [0, 1]
        const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
        double in_max = 0.0;
        for (int c = 0; c < 3; ++c) in_max = std::fmax(in_max, std::fmax(mean[c], 1.0 - mean[c]) / stdv[c]);
        v.conv1_scale = host::h2_scale_for_bound((double)v.conv[0].l1max * in_max * (1.0 + 1e-6) + v.conv[0].bmax);
    }
    for (int i = 0; i < 2; ++i) {
        const std::string p = i == 0 ? "classifier.0" : "classifier.3";
        const int k = i == 0 ? 512 * 49 : 4096;
        const float* w = sd.get(p + ".weight", (int64_t)4096 * k, err);
        const float* b = sd.get(p + ".bias", 4096, err);
        std::vector<float> rows((size_t)4096 * k);
        if (i == 0) host::vgg16_fc1_to_nhwc(w, 4096, 512, 49, rows.data());
        else std::memcpy(rows.data(), w, sizeof(float) * rows.size());
        ConvW& c = v.fc[i];
        RELAX_TRY(make_rows(h, rows, b, 4096, k, &c, v.mem, true));
        c.Cin = k; c.KH = 1; c.KW = 1; c.stride = 1; c.pad = 0;
    }
    v.loaded = true;
    return RELAX_OK;
}

// ---- forward ---------------------------------------------------------------------------------------
// One chunk of N <= kVggChunk images.  Rows of the outputs: layer_stack [N][4224], pool [N][4099], taps as in relax_vgg16_features,
// each already offset to the chunk's first image.
static int vgg_chunk(relax_handle* h, const uint8_t* frags, int N, float* layer_stack, float* pool, float* const* taps, int64_t tap_off, hipStream_t s) {
    const VggW& v = h->vgg;
    const int mode = h->gemm.precision;       // 3 f16x2, 2 bf16x6, 0 / 1 fp32 rows into the exact-fp32 (bf16x3) kernel
    const bool h2 = mode == 3, x6 = mode >= 2;
    const size_t n = (size_t)N;
    float* base = static_cast<float*>(h->arena.p);
    float* A32 = base;                                         // fp32 map in front of a max-pool, or of an export
    char* cur = reinterpret_cast<char*>(A32 + kMap * n);       // the next contraction's input (planes of the mode, or fp32 rows)
    char* oth = reinterpret_cast<char*>(A32 + (kMap + kPlanes) * n);
    float* groups = A32 + (kMap + 2 * kPlanes) * n;
    float* fc1 = groups + kGroups * n;
    float* fc2 = fc1 + kFc * n;
    float* tab = fc2 + kFc * n;
    int next_slot = 0;
    auto new_slot = [&](int* slot) -> int {   // checked before anything writes the table
        RELAX_REQUIRE(h, next_slot < kVggSlots, "vgg16: per-image scale slot %d requested, %d reserved", next_slot, kVggSlots);
        *slot = next_slot++;
        return RELAX_OK;
    };
    auto slot_amax = [&](int t) { return reinterpret_cast<unsigned*>(tab + (size_t)(3 * t) * n); };
    auto slot_scale = [&](int t) { return tab + (size_t)(3 * t + 1) * n; };
    auto slot_inv = [&](int t) { return tab + (size_t)(3 * t + 2) * n; };
    RELAX_HIP_CHECK(h, fill_async(tab, 0, sizeof(float) * 3 * kVggSlots * n, s));

    int off = 0;   // layer-stack column of the current tap
    auto tap_out = [&](int i, const float* f32, int HW, int C, int group) -> int {   // the mean (group > 0: from the fused group sums) and the export
        if (layer_stack) {
            if (group > 0) RELAX_TRY(launch_gap_groups_finish_rows(h, groups, layer_stack + off, N, HW, C, RELAX_VGG16_LAYER_STACK_DIM, group, s));
            else RELAX_TRY(launch_gap(h, f32, layer_stack + off, N, HW, C, RELAX_VGG16_LAYER_STACK_DIM, s));
        }
        if (taps && taps[i]) RELAX_TRY(launch_nhwc_to_nchw(h, f32, taps[i] + tap_off * C * HW, N, HW, C, s));
        off += C;
        return RELAX_OK;
    };

    // conv1_1
    const bool export0 = taps && taps[0];
    int s_in = -1;                 // slot of the current input tensor (f16x2: its scale; its maximum is amax_in)
    unsigned* amax_in = nullptr;
    if (h2) {
        RELAX_TRY(new_slot(&s_in));
        amax_in = slot_amax(s_in);
    }
    {
        float* o32 = x6 ? (export0 ? A32 : nullptr) : reinterpret_cast<float*>(cur);
        hipLaunchKernelGGL(vgg_conv1_1, dim3(224 * 224 / kC11Pix, N), dim3(256), 0, s, frags, v.conv[0].w, v.conv[0].bias, o32,
                           h2 ? cur : nullptr, v.conv1_scale, (x6 && !h2) ? cur : nullptr, layer_stack ? groups : nullptr, amax_in,
                           h2 ? slot_scale(s_in) : nullptr, h2 ? slot_inv(s_in) : nullptr);
        RELAX_HIP_CHECK(h, hipGetLastError());
        RELAX_TRY(tap_out(0, o32, 224 * 224, 64, 16));
    }
    for (int i = 1; i < host::kVggConvs; ++i) {
        const ConvW& c = v.conv[i];
        const int H = kVggHW[i], HW = H * H, C = c.Cout;
        const bool pool_next = kVggPoolAfter[i];
        const bool want_export = taps && taps[i];
        float* o32 = x6 ? ((pool_next || want_export) ? A32 : nullptr) : reinterpret_cast<float*>(oth);
        void* oplanes = (x6 && !pool_next) ? oth : nullptr;
        float* gap = (x6 && layer_stack) ? groups : nullptr;
        int group = 0;
        int s_out = -1;
        if (h2) {   // the output's scale from Hoelder on the measured input maximum, fixed before the launch; its own maximum is measured
            RELAX_TRY(new_slot(&s_out));
            RELAX_TRY(launch_h2_image_scales(h, amax_in, c.l1max, nullptr, 0.f, nullptr, c.bmax, slot_scale(s_out), slot_inv(s_out), N, s));
        }
        if (h2 && C % 256 == 0) {   // gemm_h3, convolution form (conv3_x .. conv5_x)
            GemmDescH2 g{};
            g.a = cur; g.w = c.w_h2; g.colscale = c.w_inv; g.bias = c.bias; g.act = 1;
            g.pixels = 1; g.Nimg = N; g.H = H; g.W = H; g.Cin = c.Cin; g.Ho = H; g.Wo = H;
            g.KH = 3; g.KW = 3; g.stride = 1; g.pad = 1;
            g.M = N * HW; g.N = C; g.K = c.Kpad;
            g.rows_per_img = HW; g.img_in_inv = slot_inv(s_in);
            g.out = o32; g.out_h2 = oplanes; g.img_out_scale = oplanes ? slot_scale(s_out) : nullptr; g.amax_out = slot_amax(s_out);
            g.gap_groups = gap;
            g.no_split = true;    // the pool vector's bits do not depend on whether the layer stack is requested
            RELAX_TRY(launch_gemm_h2(h, g, s));
            group = 4;
        } else if (x6) {            // gemm_x6: f16x2 on the four-wave tiles (64 / 128 channels) or bf16x6
            ConvDescX6 d{};
            d.in = cur; d.Nimg = N; d.H = H; d.W = H; d.Cin = c.Cin; d.Ho = H; d.Wo = H;
            d.KH = 3; d.KW = 3; d.stride = 1; d.pad = 1;
            d.Cout = C; d.bias = c.bias; d.act = 1;
            d.out = o32; d.gap_groups = gap; d.no_split = true;
            if (h2) {
                d.in_h2 = 1; d.w = c.w_h2; d.colscale = c.w_inv; d.img_in_inv = slot_inv(s_in);
                d.out_h2 = oplanes; d.img_out_scale = oplanes ? slot_scale(s_out) : nullptr; d.amax_out = slot_amax(s_out);
            } else {
                d.w = c.w_sp3; d.out_sp3 = oplanes;
            }
            RELAX_TRY(launch_conv_x6(h, d, s));
            group = HW % 16 == 0 ? 16 : 4;
        } else {
            ConvDesc d{};
            d.in = reinterpret_cast<const float*>(cur); d.Nimg = N; d.H = H; d.W = H; d.Cin = c.Cin; d.Ho = H; d.Wo = H;
            d.KH = 3; d.KW = 3; d.stride = 1; d.pad = 1;
            d.w = c.w; d.Cout = C; d.Kpad = c.Kpad; d.bias = c.bias; d.out = o32; d.act = 1;
            RELAX_TRY(launch_conv(h, d, s));
        }
        RELAX_TRY(tap_out(i, o32, HW, C, gap ? group : 0));
        if (h2) { s_in = s_out; amax_in = slot_amax(s_out); }
        if (pool_next) {
            // 2x2 max-pool of the fp32 map into `cur` (its input has been consumed): fp16 planes with the scale of the measured maximum of
            // the map (the pool's outputs are a subset of its values, so the same maximum bounds them), split planes, or fp32 rows
            const int Ho = H / 2;
            const int64_t threads = (int64_t)N * Ho * Ho * C / 8;
            const dim3 grid((unsigned)((threads + 255) / 256));
            if (h2) {
                int s_p = -1;
                RELAX_TRY(new_slot(&s_p));
                RELAX_TRY(launch_h2_image_scales(h, amax_in, 1.f, nullptr, 0.f, nullptr, 0.f, slot_scale(s_p), slot_inv(s_p), N, s));
                hipLaunchKernelGGL(vgg_maxpool2x2<1>, grid, dim3(256), 0, s, o32, cur, slot_scale(s_p), N, H, H, C);
                s_in = s_p;   // (amax_in stays: the maximum of the map)
            } else if (x6) {
                hipLaunchKernelGGL(vgg_maxpool2x2<2>, grid, dim3(256), 0, s, o32, cur, nullptr, N, H, H, C);
            } else {
                hipLaunchKernelGGL(vgg_maxpool2x2<0>, grid, dim3(256), 0, s, o32, cur, nullptr, N, H, H, C);
            }
            RELAX_HIP_CHECK(h, hipGetLastError());
        } else {
            char* t = cur; cur = oth; oth = t;
        }
    }
    // classifier: pool5 (NHWC flatten, `cur`) -> fc1 + ReLU -> fc2 + ReLU (Dropout: identity in eval)
    const bool want_fc1 = taps && taps[13], want_fc2 = taps && taps[14];
    if (!pool && !want_fc1 && !want_fc2) return RELAX_OK;
    for (int i = 0; i < 2; ++i) {
        const ConvW& c = v.fc[i];
        const bool last = i == 1;
        float* o32 = i == 0 ? fc1 : fc2;
        const bool need32 = last || want_fc1 || !x6;
        void* oplanes = (x6 && !last) ? oth : nullptr;
        if (h2) {   // a 1x1 convolution over N images of 1x1 pixels: the per-image scales of the convolution form
            int s_out = -1;
            RELAX_TRY(new_slot(&s_out));
            RELAX_TRY(launch_h2_image_scales(h, amax_in, c.l1max, nullptr, 0.f, nullptr, c.bmax, slot_scale(s_out), slot_inv(s_out), N, s));
            GemmDescH2 g{};
            g.a = cur; g.w = c.w_h2; g.colscale = c.w_inv; g.bias = c.bias; g.act = 1;
            g.pixels = 1; g.Nimg = N; g.H = 1; g.W = 1; g.Cin = c.Cin; g.Ho = 1; g.Wo = 1;
            g.KH = 1; g.KW = 1; g.stride = 1; g.pad = 0;
            g.M = N; g.N = 4096; g.K = c.Cin;
            g.rows_per_img = 1; g.img_in_inv = slot_inv(s_in);
            g.out = need32 ? o32 : nullptr; g.out_h2 = oplanes; g.img_out_scale = oplanes ? slot_scale(s_out) : nullptr;
            g.amax_out = oplanes ? slot_amax(s_out) : nullptr;
            g.no_split = true;
            RELAX_TRY(launch_gemm_h2(h, g, s));
            s_in = s_out;
            amax_in = slot_amax(s_out);
        } else if (x6) {
            ConvDescX6 d{};
            d.in = cur; d.Nimg = 1; d.H = 1; d.W = N; d.Cin = c.Cin; d.Ho = 1; d.Wo = N;
            d.KH = 1; d.KW = 1; d.stride = 1; d.pad = 0;
            d.w = c.w_sp3; d.Cout = 4096; d.bias = c.bias; d.act = 1;
            d.out = need32 ? o32 : nullptr; d.out_sp3 = oplanes; d.no_split = true;
            RELAX_TRY(launch_conv_x6(h, d, s));
        } else {
            const float* a = i == 0 ? reinterpret_cast<const float*>(cur) : fc1;
            RELAX_TRY(launch_gemm(h, a, c.w, c.bias, nullptr, o32, N, 4096, c.Cin, 1, s));
        }
        if (taps && taps[13 + i])
            RELAX_HIP_CHECK(h, hipMemcpyAsync(taps[13 + i] + tap_off * 4096, o32, sizeof(float) * 4096 * n, hipMemcpyDeviceToDevice, s));
        if (oplanes) { char* t = cur; cur = oth; oth = t; }
    }
    if (pool) RELAX_TRY(launch_pool_stats(h, fc2, 4096, pool, RELAX_VGG16_POOL_DIM, N, 4096, s));
    return RELAX_OK;
}

}  // namespace relax

using namespace relax;

extern "C" {

int relax_load_vgg16(relax_handle* h, const float* const* tensors, const char* const* names, const int64_t* numels, int n) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, tensors && names && numels && n > 0, "relax_load_vgg16: bad arguments");
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    free_vgg(h);
    host::StateDict sd;
    for (int i = 0; i < n; ++i) sd.add(names[i], tensors[i], numels[i]);
    const int rc = load_vgg(h, sd);
    if (rc != RELAX_OK) free_vgg(h);
    return rc;
}

int relax_vgg16_features(relax_handle* h, const uint8_t* frags, int N, float* layer_stack, float* pool, float* const* taps_nchw,
                         relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, h->vgg.loaded, "relax_vgg16_features: call relax_load_vgg16 first");
    RELAX_REQUIRE(h, frags && N > 0, "relax_vgg16_features: bad arguments");
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    RELAX_TRY(ensure_buf(h, h->arena, vgg_arena_bytes(N)));
    for (int i0 = 0; i0 < N; i0 += kVggChunk) {
        const int c = N - i0 < kVggChunk ? N - i0 : kVggChunk;
        RELAX_TRY(vgg_chunk(h, frags + (int64_t)i0 * 224 * 224 * 3, c, layer_stack ? layer_stack + (int64_t)i0 * RELAX_VGG16_LAYER_STACK_DIM : nullptr,
                            pool ? pool + (int64_t)i0 * RELAX_VGG16_POOL_DIM : nullptr, taps_nchw, i0, s));
    }
    return RELAX_OK;
}

}  // extern "C"
