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
// Images go through in chunks of at most host::kVggChunk (the 224^2 x 64 maps are 12.8 MB per image in fp32).
#include <cmath>

#include "relax_internal.h"
#include "host_logic.h"
#include "h2.h"
#include "sp3.h"

namespace relax {

// the arena of a call (host_logic.cpp's vgg_arena: ~1.7 GB for a whole chunk)
size_t vgg_arena_bytes(int n) { return (size_t)host::vgg_arena_bytes(n); }

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
// Where a step's tensors lie and which table rows it reads and writes: the plan's buffer and slot numbers as pointers of this chunk
struct VggIo {
    const void* in;
    float* out32;
    void* planes;
    float* gap;                  // group sums of the fused mean, or null
    const float* in_inv;         // f16x2: 1 / scale of the input planes, scale of the output planes, the output's measured maximum
    const float* out_scale;
    unsigned* out_max;
};

// One contraction step (a convolution over N maps, or a classifier layer) on the kernel of its route
static int vgg_contract(relax_handle* h, const host::VggLayerPlan& q, const ConvW& c, int N, const VggIo& io, hipStream_t s) {
    int Nimg = N, H = q.side, W = q.side;
    // a classifier layer is a plain GEMM over N rows - but on gemm_h3 a 1x1 convolution over N images of 1x1 pixels, whose scales are per image
    if (q.side == 1 && q.route != host::kVggConvH3) { Nimg = 1; W = N; }
    switch (q.route) {
        case host::kVggConvH3: {
            GemmDescH2 g = conv_h2(c, io.in, Nimg, H, W, 1);
            g.img_in_inv = io.in_inv;
            g.out = io.out32; g.out_h2 = io.planes; g.img_out_scale = io.planes ? io.out_scale : nullptr; g.amax_out = io.out_max;
            g.gap_groups = io.gap; g.no_split = q.no_split;
            return launch_gemm_h2(h, g, s);
        }
        case host::kVggConvX6H2:
        case host::kVggConvX6: {
            ConvDescX6 d = conv_x6(c, io.in, Nimg, H, W, 1);
            d.out = io.out32; d.gap_groups = io.gap; d.no_split = q.no_split;
            if (q.route == host::kVggConvX6H2) {
                d.in_h2 = 1; d.w = c.w_h2; d.colscale = c.w_inv; d.img_in_inv = io.in_inv;
                d.out_h2 = io.planes; d.img_out_scale = io.planes ? io.out_scale : nullptr; d.amax_out = io.out_max;
            } else {
                d.out_sp3 = io.planes;
            }
            return launch_conv_x6(h, d, s);
        }
        default:   // kVggConvF32
            return launch_conv(h, conv_f32(c, static_cast<const float*>(io.in), Nimg, H, W, nullptr, io.out32, 1), s);
    }
}

// One chunk of N <= host::kVggChunk images: host::vgg_plan (CPU-tested) decides every step, here are the pointers and the launches.  Rows of the
// outputs: layer_stack [N][4224], pool [N][4099], taps as in relax_vgg16_features, each already offset to the chunk's first image.
static int vgg_chunk(relax_handle* h, const uint8_t* frags, int N, float* layer_stack, float* pool, float* const* taps, int64_t tap_off, hipStream_t s) {
    const VggW& v = h->vgg;
    host::VggRequest rq{N, layer_stack != nullptr, pool != nullptr, 0u};
    for (int t = 0; taps && t < host::kVggTaps; ++t) rq.taps |= taps[t] ? 1u << t : 0u;
    host::VggPlan plan;
    std::string plan_err;
    RELAX_REQUIRE(h, host::vgg_plan(host::VggOptions{h->gemm.precision}, rq, host::kVggSlots, &plan, plan_err), "%s", plan_err.c_str());
    const size_t n = (size_t)N;
    float* base = static_cast<float*>(h->arena.p);
    const host::VggArena& a = plan.arena;
    void* const buf[] = {nullptr, base + a.a32 * n, base + a.planes0 * n, base + a.planes1 * n, base + a.fc1 * n, base + a.fc2 * n};   // by host::VggBuffer
    float* groups = base + a.groups * n;
    float* tab = base + a.slots * n;       // slot t = {maximum, scale, 1 / scale} x images
    auto slot_max = [&](int t) { return t < 0 ? nullptr : reinterpret_cast<unsigned*>(tab + (size_t)(3 * t) * n); };
    auto slot_scale = [&](int t) { return t < 0 ? nullptr : tab + (size_t)(3 * t + 1) * n; };
    auto slot_inv = [&](int t) { return t < 0 ? nullptr : tab + (size_t)(3 * t + 2) * n; };
    RELAX_HIP_CHECK(h, fill_async(tab, 0, sizeof(float) * 3 * host::kVggSlots * n, s));

    int off = 0;   // layer-stack column of the current tap
    for (int r = 0; r < plan.n_rows; ++r) {
        const host::VggLayerPlan& q = plan.row[r];
        const bool pooling = host::vgg_is_pool(q.route), fc = q.layer >= host::kVggConvs;
        const ConvW& c = fc ? v.fc[q.layer - host::kVggConvs] : v.conv[q.layer];
        const int H = q.side, HW = H * H, C = q.cout;
        const VggIo io{buf[q.in], static_cast<float*>(buf[q.out32]), buf[q.out_planes], q.gap_group ? groups : nullptr,
                       slot_inv(q.s_in), slot_scale(q.s_out), q.measure_max ? slot_max(q.s_out) : nullptr};
        // f16x2: the output's scale is fixed before the launch, from Hoelder's bound on the measured maximum of the producer's input - a pool's
        // from the measured maximum of the map it reads, which its outputs cannot pass
        if (q.s_out >= 0 && q.s_in_max >= 0)
            RELAX_TRY(launch_h2_image_scales(h, slot_max(q.s_in_max), pooling ? 1.f : c.l1max, nullptr, 0.f, nullptr, pooling ? 0.f : c.bmax,
                                             slot_scale(q.s_out), slot_inv(q.s_out), N, s));
        if (pooling) {
            const int64_t threads = (int64_t)N * (H / 2) * (H / 2) * C / 8;
            const dim3 grid((unsigned)((threads + 255) / 256));
            const float* x = static_cast<const float*>(io.in);
            if (q.route == host::kVggPoolH2) hipLaunchKernelGGL(vgg_maxpool2x2<1>, grid, dim3(256), 0, s, x, io.planes, io.out_scale, N, H, H, C);
            else if (q.route == host::kVggPoolSp3) hipLaunchKernelGGL(vgg_maxpool2x2<2>, grid, dim3(256), 0, s, x, io.planes, nullptr, N, H, H, C);
            else hipLaunchKernelGGL(vgg_maxpool2x2<0>, grid, dim3(256), 0, s, x, io.out32, nullptr, N, H, H, C);
            RELAX_HIP_CHECK(h, hipGetLastError());
            continue;
        }
        if (q.route == host::kVggConv11) {   // its planes are fp16 with the static scale where the plan gives it a slot, else split planes
            const bool h2 = q.s_out >= 0;
            hipLaunchKernelGGL(vgg_conv1_1, dim3(224 * 224 / kC11Pix, N), dim3(256), 0, s, frags, c.w, c.bias, io.out32,
                               h2 ? static_cast<char*>(io.planes) : nullptr, v.conv1_scale, h2 ? nullptr : static_cast<char*>(io.planes), io.gap,
                               io.out_max, slot_scale(q.s_out), slot_inv(q.s_out));
            RELAX_HIP_CHECK(h, hipGetLastError());
        } else {
            RELAX_TRY(vgg_contract(h, q, c, N, io, s));
        }
        if (fc) {
            if (q.want_export)
                RELAX_HIP_CHECK(h, hipMemcpyAsync(taps[q.layer] + tap_off * C, io.out32, sizeof(float) * C * n, hipMemcpyDeviceToDevice, s));
            continue;
        }
        if (q.want_mean) {   // from the fused group sums, or over the fp32 copy
            if (q.gap_group > 0) RELAX_TRY(launch_gap_groups_finish_rows(h, groups, layer_stack + off, N, HW, C, RELAX_VGG16_LAYER_STACK_DIM, q.gap_group, s));
            else RELAX_TRY(launch_gap(h, io.out32, layer_stack + off, N, HW, C, RELAX_VGG16_LAYER_STACK_DIM, s));
        }
        if (q.want_export) RELAX_TRY(launch_nhwc_to_nchw(h, io.out32, taps[q.layer] + tap_off * C * HW, N, HW, C, s));
        off += C;
    }
    if (pool) RELAX_TRY(launch_pool_stats(h, static_cast<float*>(buf[host::kVggBufFc2]), 4096, pool, RELAX_VGG16_POOL_DIM, N, 4096, s));
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
    for (int i0 = 0; i0 < N; i0 += host::kVggChunk) {
        const int c = N - i0 < host::kVggChunk ? N - i0 : host::kVggChunk;
        RELAX_TRY(vgg_chunk(h, frags + (int64_t)i0 * 224 * 224 * 3, c, layer_stack ? layer_stack + (int64_t)i0 * RELAX_VGG16_LAYER_STACK_DIM : nullptr,
                            pool ? pool + (int64_t)i0 * RELAX_VGG16_POOL_DIM : nullptr, taps_nchw, i0, s));
    }
    return RELAX_OK;
}

}  // extern "C"
