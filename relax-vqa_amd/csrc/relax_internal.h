// Internal declarations shared by the translation units of librelax_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <map>
#include <string>
#include <vector>

#include "host_logic.h"
#include "relax_hip.h"

namespace relax {

constexpr int kMaxDevices = 64;   // relax_create refuses device ids beyond this (per-device launch-attribute flags)

// ---- error plumbing -------------------------------------------------------------------------
void set_error(relax_handle* h, const char* fmt, ...);

#define RELAX_HIP_CHECK(h, expr)                                                             \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            relax::set_error((h), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return RELAX_ERR_HIP;                                                            \
        }                                                                                    \
    } while (0)

#define RELAX_REQUIRE(h, cond, ...)                                                          \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            relax::set_error((h), __VA_ARGS__);                                              \
            return RELAX_ERR_INVALID;                                                        \
        }                                                                                    \
    } while (0)

#define RELAX_TRY(expr)                                                                      \
    do {                                                                                     \
        int rc_ = (expr);                                                                    \
        if (rc_ != RELAX_OK) return rc_;                                                     \
    } while (0)

// ---- byte-wise |a - b| of four packed uint8 (cv2.absdiff): the fragment gather and the pair resize ------
__device__ inline uint32_t absdiff_u8x4(uint32_t a, uint32_t b) {
    uint32_t r = 0;
#pragma unroll
    for (int s = 0; s < 32; s += 8) {
        const int x = (a >> s) & 255, y = (b >> s) & 255;
        r |= (uint32_t)(x > y ? x - y : y - x) << s;
    }
    return r;
}

// ---- device buffers -------------------------------------------------------------------------
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

// device memory that lives as long as a loaded model (or a training state): every pointer is recorded the moment its allocation succeeds, so
// a load that fails half-way gives back exactly what it took (api.hip)
struct DeviceOwner {
    std::vector<void*> ptrs;
    void* keep(relax_handle* h, size_t bytes, const char* what);            // nullptr and a message naming `what` and the size on failure
    int upload(relax_handle* h, const float* host, size_t n, float** dev);  // keep + copy of n floats
    void release();                                                         // frees everything kept
};

// fp32 staging rows of a weight conversion: device memory freed at the end of the scope
struct ScopedDev {
    float* p = nullptr;
    bool alloc(relax_handle* h, size_t floats, const char* what);   // false and a message on failure
    ~ScopedDev();
};

// ---- contraction kernel description -----------------------------------------------------------
struct ConvDesc {
    // A operand: NHWC activation, gathered on the fly (implicit GEMM)
    const float* in;
    int Nimg, H, W, Cin;
    int Ho, Wo;
    int KH, KW, stride, pad;
    // B operand: weights [Cout][Kpad], k = (dy*KW+dx)*Cin + c, zero padded to Kpad (% 32 == 0)
    const float* w;
    int Cout, Kpad;
    // epilogue
    const float* bias;      // [Cout] or null
    const float* residual;  // [M, Cout] or null
    float* out;             // [M, Cout]
    int act;                // 0 none, 1 relu, 2 gelu(erf)
    double flops;           // algorithmic FLOPs for the profiler (0 = 2*M*N*KH*KW*Cin)
};

// sp3 ("split planes") operands of the bf16x6 kernel (gemm_x6.hip): every fp32 value as bf16 hi + mid + lo, a row of K
// values = K/16 chunks of [16 hi][16 mid][16 lo] (96 bytes)
struct ConvDescX6 {
    const void* in;         // sp3 NHWC activation [Nimg*H*W][Cin*6 B] (plain GEMM: H = 1, W = M rows of Cin = K values)
    int Nimg, H, W, Cin;
    int Ho, Wo;
    int KH, KW, stride, pad;
    const void* w;          // sp3 weights [Cout][KH*KW*Cin*6 B], k = (dy*KW+dx)*Cin + c  (with in2: [Cout][(Cin + Cin2)*6 B])
    int Cout;
    // optional second activation source of a 1x1 contraction (ResNet downsample branch folded into conv3: one accumulator
    // sums W3 t2 + Wd x): sp3 NHWC [Nimg*H2*W2][Cin2*6 B], sampled at (oy, ox) * stride2; the weight rows are concatenated
    const void* in2;
    int H2, W2, Cin2, stride2;
    int in_f32;             // 1: `in` is plain fp32 [M][Cin] rows (split into planes inside the K loop): 1x1 stride-1, Cout = 64 / 128 only
    // f16x2 on the four-wave tiles (the 3x3 convolutions of layer1 / layer2): `in` and `w` are two fp16 planes (csrc/h2.h: [..][Cin*4 B],
    // [Cout][K*4 B]), image i's activations scaled by 1 / img_in_inv[i], weight row n by 1 / colscale[n]; Cout = 64 / 128, K >= 256
    int in_h2;
    const float* colscale;
    const float* img_in_inv;
    // ... and with in_f32 (1x1, Cout = 64 / 128, K >= 256): `in` stays fp32 rows, `w` is fp16 planes; the rows are split into planes inside the K loop
    // with image i's scale img_in_scale[i] (from its MEASURED maximum: launch_h2_image_scales with la = 1), img_in_inv = 1 / that
    const float* img_in_scale;
    int out_rows, gap_rows; // rows below these limits get the fp32 output / the group sums (0 = all rows)
    bool no_split;          // never cut tail tiles along K (a launch whose bits must not depend on which outputs are requested)
    const float* bias;      // [Cout] or null
    const float* residual;  // fp32 [M, Cout] or null
    const void* residual_sp3;  // the residual as split planes instead (exact), or null
    float* gap_groups;      // fused spatial mean, stage 1: sums over aligned 16-row groups [M/16][Cout] (Ho*Wo % 16 != 0: 4-row groups [M/4][Cout]), or null
    float* out;             // fp32 [M, Cout] or null
    void* out_sp3;          // sp3 [M][Cout*6 B] or null (at least one output)
    // the hand-over to the f16x2 convolutions of layer3 (gemm_h2.hip, "per-image scales"): the outputs also as two fp16 planes with
    // image i's rows scaled by img_out_scale[i], and / or the per-image maximum of the (non-negative) outputs; both run unsplit
    void* out_h2;
    const float* img_out_scale;
    unsigned* amax_out;
    int act;                // 0 none, 1 relu, 2 gelu(erf)
    double flops;           // algorithmic FLOPs for the profiler (0 = 2*M*N*K)
    // back-to-back form ("rn_fuse", with in_h2): the 3x3 convolution's output tile (bias + ReLU applied) never leaves the CU - it is the A
    // operand of the block's conv3, a 1x1 onto Cout3 columns with K = Cout.  `bias` is then the 3x3's, act must be 1, and residual /
    // out / out_rows / out_sp3 / out_h2 / img_out_scale / amax_out / gap_groups / gap_rows describe the conv3 output [M][Cout3]
    // (ReLU behind the residual add).  w3: h2 weights [Cout3][Cout*4 B] whose K axis is in the accumulator order of the 3x3's
    // transposed tile (launch_b2b_permute_k), colscale3 their inverse row scales, bias3 [Cout3].
    const void* w3;
    const float* colscale3;
    const float* bias3;
    int Cout3;
    const float* x2;        // back-to-back form of a layer's FIRST block (64-wide): the block input as fp32 rows [M][64] - conv3 then contracts over
                            // K = [the 3x3's 64 channels | these 64] with w3 = [conv3 (permuted K) | downsample (natural K)] rows of 128 and bias3 = the sum of
                            // the two shifts; no residual
    int sp3_sub;            // back-to-back form: 2 = out_sp3 receives only the pixels with even (oy, ox), as compact [Nimg][Ho/2][Wo/2] rows - the sample the
                            // next block's stride-2 downsample branch reads (the full map travels as fp32 rows); 0 / 1 = every pixel
};

// h2 ("two fp16 planes", csrc/h2.h) operands of the f16x2 kernel (gemm_h2.hip): plain GEMM, N % 256 == 0
struct GemmDescH2 {
    const void* a;          // h2 activations [M][K*4 B], values scaled by a power of two
    const void* w;          // h2 weights [N][K*4 B], row n scaled by 2^t_n
    const float* colscale;  // [N]: the inverse of (weight row scale x static activation scale)
    const float* rowscale;  // [M]: the inverse of a per-row activation scale, or null
    const float* bias;      // [N] or null
    const float* residual;  // fp32 [M][N] or null
    float* out;             // fp32 [M][N] or null
    void* out_h2;           // h2 [M][N*4 B] or null (at least one output), values scaled by out_scale (a power of two from a bound)
    float out_scale;
    int M, N, K;
    int act;                // 0 none, 1 relu, 2 gelu(erf)
    bool no_split;
    // convolution form (gemm_h3 as implicit GEMM; ResNet-50 layer3 / layer4): a = NHWC planes [Nimg*H*W][Cin*4 B], M = Nimg*Ho*Wo,
    // K = KH*KW*Cin, weight rows k = (dy*KW + dx)*Cin + c; pixels = 0: plain GEMM
    int pixels, Nimg, H, W, Cin, Ho, Wo, KH, KW, stride, pad;
    // per-image scales (image = row / rows_per_img) and the per-image maximum of the outputs (see h2_image_scales)
    int rows_per_img;
    const float* img_in_inv;
    const float* img_out_scale;
    unsigned* amax_out;
    const void* residual_h2;      // the residual as fp16 planes [M][N*4 B] with img_res_inv[image] (instead of `residual`), or null
    const float* img_res_inv;
    float* gap_groups;            // fused spatial mean, stage 1: sums over aligned 4-row groups [M/4][N], or null
    int out_rows, gap_rows;       // rows below these limits get the fp32 output / the group sums (0 = all rows)
};

// ---- model weights ------------------------------------------------------------------------------
struct ConvW {          // one folded conv (+BN) of ResNet-50
    float* w = nullptr;     // device [Cout][Kpad]
    void* w_sp3 = nullptr;  // the same as split planes (bf16x6 kernel); conv1: [64][224], k = ky*32 + kx*3 + c (conv1_x6.hip)
    void* w_h2 = nullptr;   // layer3 / layer4: the same as two fp16 planes, row n scaled by 2^t_n (gemm_h2.hip)
    float* w_inv = nullptr; // [Cout]: 2^-t_n
    void* w_h2p = nullptr;  // conv3 of a fused layer1 / layer2 block: fp16 planes with the K axis permuted for the back-to-back form (gemm_x6.hip, B2B)
    float* w_invp = nullptr;
    float l1max = 0.f;      // max_n sum_k |W[n,k]| of the folded weights and max_n |bias[n]|: Hoelder bound of the outputs from the
    float bmax = 0.f;       // measured maximum of the inputs (per-image scales, gemm_h2.hip)
    float* bias = nullptr;  // device [Cout] (null for the raw conv1)
    int Cin = 0, Cout = 0, KH = 1, KW = 1, stride = 1, pad = 0, Kpad = 0;
};

struct Bottleneck {
    ConvW c1, c2, c3, down;
    // bf16x6 path, blocks with a downsample branch: conv3 and the downsample convolution as ONE contraction over the concatenated
    // K = [conv2 output | block input] (weights [Cout][(width + Cin) * 6 B] as split planes, bias = the sum of the two folded shifts)
    void* c3d_w_sp3 = nullptr;
    float* c3d_bias = nullptr;
    void* c3d_w_h2p = nullptr;   // back-to-back form of a 64-wide first block: [conv3 (K permuted) | downsample] rows as fp16 planes + their inverse row scales
    float* c3d_w_invp = nullptr;
    bool has_down = false;
    int tap = -1;  // layer-stack tap index, -1 if not tapped
};

struct ResNet50W {
    bool loaded = false;
    ConvW conv1;                 // Cin padded 3 -> 4, K 196 -> 224, no bias (raw tap precedes bn1)
    float* bn1_scale = nullptr;  // [64]
    float* bn1_shift = nullptr;  // [64]
    std::vector<Bottleneck> blocks;  // 16
    DeviceOwner mem;
    int canvas_h = 224, canvas_w = 224;   // the canvas the forward reads its images at (relax_resnet50_set_canvas; a load puts 224 x 224 back)
    int canvas_flags = 0;                 // the rule it was accepted under (relax_resnet50_set_canvas_ex: RELAX_RN_CANVAS_ANY; a load puts 0 back)
};

struct LinearW {
    float* w = nullptr;  // device [out][in]
    void* w_sp3 = nullptr;  // the same matrix as split planes (bf16 hi + mid + lo, gemm_x6.hip), made once at load time
    void* w_h2 = nullptr;   // the same matrix as two fp16 planes, row n scaled by 2^t_n (gemm_h2.hip), made once at load time
    float* colscale = nullptr;   // [out]: 2^-t_n / (static scale of the activation tensor this layer reads)
    float* b = nullptr;  // device [out]
    int in = 0, out = 0;
};

struct VitBlockW {
    float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    LinearW qkv, proj, fc1, fc2;
    // f16x2: static power-of-two scales of the activation tensors that travel as fp16 planes (host_logic.h: from bounds that hold
    // for every input): LayerNorm 1 output, attention output, LayerNorm 2 output, GELU(fc1) output
    float s_ln1 = 1.f, s_att = 1.f, s_ln2 = 1.f, s_hid = 1.f;
    float s_qkv = 1.f;   // ... and the whole qkv output (attention_h2.hip reads q, k, v as planes)
};

// interpolate_pos_encoding's table of one patch grid (vit_pos_interp, vit.hip): [1 + gh*gw][dim] on the device, complete when cached
struct VitPosTable {
    int gh = 0, gw = 0;
    float* table = nullptr;
    uint64_t used = 0;      // VitW::pos_clock of the last call that read it (the least recent entry is replaced)
};
constexpr int kVitPosCache = 4;

struct VitW {
    bool loaded = false;
    int dim = 0, depth = 0, heads = 0;
    float* cls = nullptr;   // [dim]
    int patch = 16, ntok = 197, npatch = 196, patch_k = 768;   // host::vit_geometry of the loaded checkpoint's patch size (8: 785 tokens)
    float* pos = nullptr;   // [ntok][dim]: the checkpoint's table, the grid of a 224 x 224 call
    VitPosTable pos_cache[kVitPosCache];   // the tables of the last few other grids (relax_vit_features_canvas, relax_vit_pos_embed); free_vit drops them
    uint64_t pos_clock = 0;
    LinearW patch_w;        // [dim][3*p*p], k = (c*p + py)*p + px (c in RGB order)
    std::vector<VitBlockW> blocks;
    float *norm_g = nullptr, *norm_b = nullptr;
    DeviceOwner mem;
};

// ---- VGG-16 (csrc/vgg16.hip) -------------------------------------------------------------------------------------------------
struct VggW {
    bool loaded = false;
    ConvW conv[13];         // conv[0]: [64][32] fp32 (k = (dy*3+dx)*3 + c, RGB, zero padded): vgg_conv1_1 reads it directly; the others as ResNet's
    ConvW fc[2];            // classifier.0 (columns permuted to the NHWC flatten of pool5) and classifier.3 as 1x1 convolutions over 1x1 images
    float conv1_scale = 1.f;   // static power of two of conv1_1's fp16-plane output (a bound from the normalised input range)
    DeviceOwner mem;
};

// ---- quality head (imputer + scaler + MLP), BatchNorm folded into fc1 ----------------------------------------
struct HeadW {
    bool loaded = false;
    int F = 0, Fpad = 0, H1 = 0, H2 = 0;
    float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr, *w3 = nullptr;
    float b3 = 0.f;
    double *stats = nullptr, *scale = nullptr, *mn = nullptr;
    DeviceOwner mem;
};

// ---- quality head, training state (head_train.hip) -----------------------------------------------------------
// One parameter set is ONE device block of floats: the parameters first (what SGD and the SWA average touch), then the BatchNorm
// buffers:  W1 [H1][Fpad] | b1 | gamma | beta | W2 [H2][H1] | b2 | w3 [H2] | b3 | running_mean [H1] | running_var [H1]
// and two int64 counters (num_batches_tracked, n_averaged).  Sets: 0 live (with the optimizer's one or two state blocks), 1 SWA average, 2 snapshot.
struct HeadTrain {
    static constexpr int kSets = 3;
    static constexpr int kMaxBatch = 1024;
    bool ready = false;
    bool batchnorm = true;            // false: the plain Mlp of model_regression_simple.py (no bn1; relax_head_train_init_ex)
    int F = 0, Fpad = 0, H1 = 0, H2 = 0, max_batch = 0;
    size_t n_params = 0, n_all = 0;   // floats of the parameter part / of the whole set
    float* set[kSets] = {};
    float* mom = nullptr;             // SGD momentum buffers / Adam's exp_avg, parameter part's layout
    float* var = nullptr;             // Adam's exp_avg_sq, the same layout; the SGD step never reads or writes it
    int64_t adam_t = 0;               // Adam's step count (torch keeps one per parameter, all equal); lives on the host: the bias
                                      // corrections of a step are computed there and passed to its kernels
    int64_t* counters = nullptr;      // [kSets][2]
    double* loss = nullptr;           // [2][3]: train / eval: sum of batch losses, sum of batch loss * batch size, batches
    float* act = nullptr;             // activations of one batch (head_train.hip lays them out)
    float* xb = nullptr;              // the gathered batch rows [max_batch][Fpad]
    float* grad_w1 = nullptr;         // dW1 of the UNFUSED form (relax_head_train_dw1 with fused = 0, a measurement): allocated on its first use
    DevBuf scaler_ws;                 // partial column sums / minima / maxima of the scaler fit
    DeviceOwner mem;
};

// ---- resize coefficient tables (Pillow-exact; resize.hip), cached per (input size, output size, filter): coeffs and bounds share one
// allocation; the least recently used of the kResizeAnyCache entries is replaced (a call needs at most four)
struct ResizeAnyTable {
    int in_size = 0, out_size = 0, filt = 0, kstride = 0;
    int32_t* coeffs = nullptr;  // device [out_size][kstride]: the table's rows padded with zeros to a multiple of four taps (16-byte rows)
    int32_t* bounds = nullptr;  // device [out_size][2], behind coeffs
    uint64_t used = 0;          // relax_handle::resize_any_clock of the last call that read it
};
constexpr int kResizeAnyCache = 16;

// ---- event profiling ----------------------------------------------------------------------------
struct ProfSpan {
    hipEvent_t start, stop;
    double work;
    double bytes;  // algorithmic HBM bytes of the launch (contraction kernel), 0 otherwise
    int kind;
    bool ended;    // prof_end has re-recorded `stop` (an open span - the Farneback stage around its kernels' spans - is never reaped)
};

struct Profiler {
    bool on = false;
    std::vector<ProfSpan> spans;   // span_idx handed out by prof_begin = span_base + position here
    int span_base = 0;             // spans reaped so far (prof_begin folds finished spans into the totals once kReapAt have piled up:
                                   // a pass of thousands of clips with the profiler on keeps a bounded number of HIP events)
    static constexpr size_t kReapAt = 2048;
    std::vector<hipEvent_t> pool;
    // span kinds: 0 fp32 / bf16x3 contraction, 1 patch score, 2 bf16x6 contraction, 3 Farneback iteration kernel, 4 the whole Farneback stage,
    // 5 f16x2 contraction, convolution form (gemm_h2.hip, gemm_x6<H2>, conv1_x6<H2>, the fused blocks), 6 f16x2 plain GEMMs (the ViT's: the dominant kernel)
    static constexpr int kKinds = 7;
    double total_ms[kKinds] = {};
    double total_work[kKinds] = {};
    double total_bytes[kKinds] = {};
    int64_t launches[kKinds] = {};
};

}  // namespace relax

struct relax_handle {
    int device = 0;
    relax::GemmOptions gemm;
    std::string last_error;
    relax::DevBuf arena;        // activation workspace shared by both backbones
    int reserved_images = 0;
    relax::DevBuf scratch;      // stage-A scratch (scores)
    relax::DevBuf splitk_ws;    // split-K partial tiles of the contraction kernel
    relax::DevBuf sp3_ws;       // operand conversions of the operator-level entry points under "bf16x6"
    relax::DevBuf resize_ws;    // uint8 intermediates of the two-pass resize
    relax::DevBuf flow_ws;      // optical-flow pyramid workspace
    relax::DevBuf head_ws;      // scaled features + hidden activations of the quality head
    relax::DevBuf metrics_ws;   // pair counters and results of the correlation metrics (metrics.hip)
    relax::HeadW head;
    relax::HeadTrain head_train;
    relax::ResizeAnyTable resize_any_cache[relax::kResizeAnyCache];
    uint64_t resize_any_clock = 0;
    relax::ResNet50W rn;
    relax::VitW vit;
    relax::VggW vgg;
    relax::Profiler prof;
};

namespace relax {

int ensure_buf(relax_handle* h, DevBuf& b, size_t bytes);

// hipMemsetAsync's place on every path a caller may capture into a graph: `bytes` bytes of `value` at p, by a kernel of this library on `s`
// (api.hip).  A memset NODE of a few hundred bytes wrote other bytes than asked for from the second replay of its graph on (seen with
// 64 and 1152 bytes, not with 1 MiB; tests/test_gpu_stream_contract.py replays twice); a kernel node carries its arguments itself.
hipError_t fill_async(void* p, int value, size_t bytes, hipStream_t s);

// The opt-in of a launch site's kernel (or of the instantiations it chooses among) to `bytes` of dynamic LDS - more than the 64 KB a launch
// gets unasked -, once per site and device (api.hip).  `done` is the site's own flags [kMaxDevices]: the attribute lives on the device's code
// object, per kernel instantiation, so inside a templated launcher the array is a function-local static of that instantiation.  Atomic: two
// handles of one device may launch from two threads (the call is idempotent, so the worst a lost race does is set the attribute twice); the
// flag is stored only after every call has succeeded.
int allow_dynamic_lds(relax_handle* h, std::initializer_list<const void*> kernels, size_t bytes, std::atomic<bool>* done);

// The tile grid and the tail split-K of a contraction launch (gemm.hip, gemm_x6.hip, gemm_h2.hip: their parameter structs share the field
// names): BM x BN tiles over `slots` resident workgroups, `nk` K steps of which a slice keeps at least `min_steps`.  The last, partial round of
// tiles would leave most CUs idle; where the launch can be split, those tiles are cut along K so that the tail fills the chip once with short
// work units (cost model: host::choose_tail_split; the launcher's finish kernel sums the partial tiles in order).  An unsplit launch is
// {full_tiles = ntiles, nsplit = 1}, which is what choose_tail_split returns when it does not split.
constexpr size_t kSplitKWsFloor = (size_t)(64 << 20);   // the least splitk_ws is requested at (head_train.hip too)
template <class Params>
int plan_tiles(relax_handle* h, Params& p, int BM, int BN, int slots, int nk, int min_steps, bool can_split) {
    p.tiles_n = p.N / BN;
    p.tiles_m = (p.M + BM - 1) / BM;
    p.ntiles = p.tiles_m * p.tiles_n;
    p.group_m = h->gemm.group_m;
    const host::TailSplit ts = host::choose_tail_split(p.ntiles, slots, nk, min_steps, can_split);
    p.full_tiles = ts.full_tiles;
    p.nsplit = ts.nsplit;
    p.partial = nullptr;
    if (p.nsplit > 1) {
        const size_t need = sizeof(float) * (size_t)(p.ntiles - p.full_tiles) * p.nsplit * BM * BN;
        RELAX_TRY(ensure_buf(h, h->splitk_ws, need < kSplitKWsFloor ? kSplitKWsFloor : need));
        p.partial = static_cast<float*>(h->splitk_ws.p);
    }
    return RELAX_OK;
}

// derived copies of a packed fp32 [rows][K] matrix on the device, kept by `mem` (weights.hip): split planes (sp3.h), and two fp16 planes with
// one power-of-two scale per row + the inverse scales (h2.h).  The conversions are enqueued on the null stream; `what` names the matrix in an
// allocation failure's message
int derive_sp3(relax_handle* h, DeviceOwner& mem, const float* w_dev, int rows, int K, void** out, const char* what);
int derive_h2_rows(relax_handle* h, DeviceOwner& mem, const float* w_dev, int rows, int K, void** planes, float** inv, const char* what);

// profiling helpers: call around a launch; no-ops when profiling is off
int prof_begin(relax_handle* h, hipStream_t s, int kind, double work, int* span_idx, double bytes = 0);
int prof_end(relax_handle* h, hipStream_t s, int span_idx);
void prof_set_work(relax_handle* h, int span_idx, double work);   // the work of an open span, known only at its end (span ids are not vector positions)
void prof_abort(relax_handle* h, int span_idx);   // a launch failed between begin and end: drop the half-recorded span

// contraction kernel launcher (gemm.hip)
int launch_conv(relax_handle* h, const ConvDesc& d, hipStream_t s);
inline int launch_gemm(relax_handle* h, const float* A, const float* W, const float* bias, const float* residual,
                       float* out, int M, int N, int K, int act, hipStream_t s) {
    ConvDesc d{};
    d.in = A; d.Nimg = 1; d.H = 1; d.W = M; d.Cin = K; d.Ho = 1; d.Wo = M;
    d.KH = 1; d.KW = 1; d.stride = 1; d.pad = 0;
    d.w = W; d.Cout = N; d.Kpad = K; d.bias = bias; d.residual = residual; d.out = out; d.act = act;
    return launch_conv(h, d, s);
}

// bf16x6 contraction kernel (gemm_x6.hip)
int launch_conv_x6(relax_handle* h, const ConvDescX6& d, hipStream_t s);
int launch_b2b_permute_k(relax_handle* h, const float* w, float* wp, int rows, int K, hipStream_t s);   // gemm_x6.hip: K order of the back-to-back form
int launch_to_sp3(relax_handle* h, const float* x, int64_t ld, void* y, int64_t rows, int K, hipStream_t s);
// conv1_x6.hip: ResNet-50 conv1 on the bf16x6 arithmetic, straight from the uint8 fragments
int make_conv1_x6_weights(relax_handle* h, const float* w_packed, int kpad, void** w_sp3_out, DeviceOwner& mem);
int launch_conv1_x6(relax_handle* h, const uint8_t* frags, const void* w_sp3, float* out, float* gap_groups, int N, int Hc, int Wc, hipStream_t s,
                    const float* w_inv = nullptr);   // frags [N,Hc,Wc,3]; w_inv: `w_sp3` holds fp16 planes and the f16x2 form runs
int make_conv1_h2_weights(relax_handle* h, const float* w_packed, int kpad, void** w_h2_out, float** w_inv_out, DeviceOwner& mem);
// the same stem on any canvas: out [N,(Hc-1)/2+1,(Wc-1)/2+1,64], partial 16 x 16 tiles, image rows at any byte alignment; gap_groups only where
// the output rows are whole 16-pixel groups (host_logic.h: rn_maps_stem_fused_mean)
int launch_conv1_x6_any(relax_handle* h, const uint8_t* frags, const void* w_sp3, float* out, float* gap_groups, int N, int Hc, int Wc, hipStream_t s,
                        const float* w_inv = nullptr);
inline int launch_gemm_x6(relax_handle* h, const void* A_sp3, const void* W_sp3, const float* bias, const float* residual,
                          float* out, void* out_sp3, int M, int N, int K, int act, hipStream_t s) {
    ConvDescX6 d{};
    d.in = A_sp3; d.Nimg = 1; d.H = 1; d.W = M; d.Cin = K; d.Ho = 1; d.Wo = M;
    d.KH = 1; d.KW = 1; d.stride = 1; d.pad = 0;
    d.w = W_sp3; d.Cout = N; d.bias = bias; d.residual = residual; d.out = out; d.out_sp3 = out_sp3; d.act = act;
    return launch_conv_x6(h, d, s);
}

// f16x2 contraction kernel (gemm_h2.hip)
int launch_gemm_h2(relax_handle* h, const GemmDescH2& d, hipStream_t s);

// Descriptors of one loaded convolution (ConvW) over Nimg maps of H x W, for the backbones (resnet50.hip, vgg16.hip): geometry, weights and
// bias; the caller adds the outputs and whatever else its launch takes.
inline int conv_out(int n, int k, int stride, int pad) { return (n + 2 * pad - k) / stride + 1; }   // output side along one axis
// the exact-fp32 (bf16x3) kernel on fp32 rows
inline ConvDesc conv_f32(const ConvW& c, const float* in, int Nimg, int H, int W, const float* residual, float* out, int act, double flops = 0) {
    ConvDesc d{};
    d.in = in; d.Nimg = Nimg; d.H = H; d.W = W; d.Cin = c.Cin;
    d.Ho = conv_out(H, c.KH, c.stride, c.pad);
    d.Wo = conv_out(W, c.KW, c.stride, c.pad);
    d.KH = c.KH; d.KW = c.KW; d.stride = c.stride; d.pad = c.pad;
    d.w = c.w; d.Cout = c.Cout; d.Kpad = c.Kpad;
    d.bias = c.bias; d.residual = residual; d.out = out; d.act = act; d.flops = flops;
    return d;
}
// gemm_x6 with the bf16x6 weights (a launch on fp16 planes replaces w and sets in_h2, colscale, img_in_inv)
inline ConvDescX6 conv_x6(const ConvW& c, const void* in_sp3, int Nimg, int H, int W, int act = 1) {
    ConvDescX6 d{};
    d.in = in_sp3; d.Nimg = Nimg; d.H = H; d.W = W; d.Cin = c.Cin;
    d.Ho = conv_out(H, c.KH, c.stride, c.pad); d.Wo = conv_out(W, c.KW, c.stride, c.pad);
    d.KH = c.KH; d.KW = c.KW; d.stride = c.stride; d.pad = c.pad;
    d.w = c.w_sp3; d.Cout = c.Cout; d.bias = c.bias; d.act = act;
    return d;
}
// gemm_h3, convolution form with per-image scales: fills geometry and weights into `g` (whose outputs the caller has set); the caller adds the
// slots of the per-image tables
inline GemmDescH2 conv_h2(const ConvW& c, const void* in_h2, int Nimg, int H, int W, int act, GemmDescH2 g = GemmDescH2{}) {
    g.a = in_h2; g.w = c.w_h2; g.colscale = c.w_inv; g.bias = c.bias; g.act = act;
    g.pixels = 1; g.Nimg = Nimg; g.H = H; g.W = W; g.Cin = c.Cin;
    g.Ho = conv_out(H, c.KH, c.stride, c.pad); g.Wo = conv_out(W, c.KW, c.stride, c.pad);
    g.KH = c.KH; g.KW = c.KW; g.stride = c.stride; g.pad = c.pad;
    g.M = Nimg * g.Ho * g.Wo; g.N = c.Cout; g.K = c.KH * c.KW * c.Cin;
    g.rows_per_img = g.Ho * g.Wo;
    return g;
}
int launch_to_h2(relax_handle* h, const float* x, int64_t ld, void* y, int64_t rows, int K, float scale, const float* row_scale, hipStream_t s,
                 int rows_per_scale = 1);
int launch_h2_image_scales(relax_handle* h, const unsigned* amax_a, float la, const unsigned* amax_b, float lb, const unsigned* amax_r,
                           float bmax, float* scale, float* inv, int n, hipStream_t s);
int launch_image_absmax(relax_handle* h, const float* x, int64_t per_image, int n_images, unsigned* amax, hipStream_t s);
int launch_to_h2_rows(relax_handle* h, const float* x, int64_t ld, void* y, int rows, int K, float* inv_scale, hipStream_t s);

// small kernels (layers.hip)
int launch_layernorm(relax_handle* h, const float* x, const float* g, const float* b, float* y, int rows, int dim,
                     float eps, hipStream_t s);
int launch_layernorm_sp3(relax_handle* h, const float* x, const float* g, const float* b, void* y_sp3, int rows, int dim,
                         float eps, hipStream_t s);
int launch_attention(relax_handle* h, const float* qkv, float* out, int Nimg, int heads, hipStream_t s);
int launch_layernorm_h2(relax_handle* h, const float* x, const float* g, const float* b, void* y_h2, float scale, int rows, int dim,
                        float eps, hipStream_t s);
// out_planes: split planes (out_h2_scale == 0) or two fp16 planes scaled by out_h2_scale (> 0)
int launch_attention_x6(relax_handle* h, const float* qkv, float* out, void* out_planes, int Nimg, int heads, hipStream_t s,
                        float out_h2_scale = 0.f);
// attention on the fp16 planes the qkv GEMM wrote (attention_h2.hip): qkv_planes [Nimg*197][3*dim*4 B] of qkv * s_qkv -> out_planes [..][dim*4 B] of out * out_scale
int launch_attention_h2(relax_handle* h, const void* qkv_planes, float s_qkv, void* out_planes, float out_scale, int Nimg, int heads, hipStream_t s);
int launch_attention_h2_op(relax_handle* h, const float* qkv, float* out, int Nimg, int heads, hipStream_t s);   // fp32 in / out (relax_op_attention)
// streaming attention for any token count (attention_stream.hip): qkv fp32 [Nimg*ntok][3*dim]; the x6 form's outputs as launch_attention_x6's
int launch_attention_stream_f32(relax_handle* h, const float* qkv, float* out, int Nimg, int ntok, int heads, hipStream_t s);
int launch_attention_stream_x6(relax_handle* h, const float* qkv, float* out, void* out_planes, int Nimg, int ntok, int heads, hipStream_t s,
                               float out_h2_scale = 0.f);
// the same on fp16 planes (attention_stream_h2.hip): attention_h2's arithmetic, operands and output layout at any token count
int launch_attention_stream_h2(relax_handle* h, const void* qkv_planes, float s_qkv, void* out_planes, float out_scale, int Nimg, int ntok, int heads,
                               hipStream_t s);
int launch_attention_stream_h2_op(relax_handle* h, const float* qkv, float* out, int Nimg, int ntok, int heads, hipStream_t s);   // fp32 in / out (relax_op_attention_ex)
// the operator entries' steps around their kernel (attention_h2.hip): fp32 qkv [rows][3 dim] -> planes with one scale from the measured maximum ->
// kernel(qkv planes, output planes, {alpha, out_mul} on the device) -> fp32 out [rows][dim]
using AttentionH2OpKernel = std::function<int(const char* qkv_planes, char* out_planes, const float* tab)>;
int attention_h2_op_steps(relax_handle* h, const float* qkv, float* out, int64_t rows, int dim, hipStream_t s, const AttentionH2OpKernel& kernel);
// the last block's CLS attention row (vit_attention_map.hip): qkv as fp32 rows [Nimg*ntok][3*dim] or, with planes, fp16 planes of
// qkv * s_qkv (csrc/h2.h) -> out fp32 [Nimg, heads, ntok] = softmax(q_0 k^T / 8) per (image, head)
// (ntok <= 4352: 256 threads x 4 keys up to 1024 tokens, x 17 above)
// the final norm of a tap of the residual stream X [Nimg, ntok, dim] without its normed tokens in HBM (csrc/vit_layers.hip): the normed CLS
// row -> cls_out [Nimg, dim], mean | max | std over the normed patch rows -> pooled_out [Nimg, 3 dim] (either may be NULL, not both)
int launch_vit_norm_token_stats(relax_handle* h, const float* X, const float* g, const float* b, float eps, float* cls_out, float* pooled_out,
                                int Nimg, int ntok, int dim, hipStream_t s);
int launch_vit_cls_attention(relax_handle* h, const void* qkv, bool planes, float s_qkv, float* out, int Nimg, int ntok, int heads, hipStream_t s);
int launch_bn_relu_maxpool(relax_handle* h, const float* x, const float* scale, const float* shift, float* y,
                           int Nimg, int H, int W, int C, hipStream_t s);
int launch_bn_relu_maxpool_f32(relax_handle* h, const float* x, const float* scale, const float* shift, float* y, int Nimg, int H, int W, int C,
                               hipStream_t s, unsigned* amax_out, unsigned* block_ws);   // fp32 rows out + the per-image maxima
int launch_bn_relu_maxpool_sp3(relax_handle* h, const float* x, const float* scale, const float* shift, void* y_sp3,
                               int Nimg, int H, int W, int C, hipStream_t s, unsigned* amax_out = nullptr, unsigned* block_ws = nullptr);
// the same max-pool on any map: out [(H-1)/2+1][(W-1)/2+1], the window clipped at all four edges.  y: fp32 rows; y_sp3: bf16 planes (one of the two);
// amax_out [Nimg]: the per-image maximum of the outputs, posted on any map (block_ws: Nimg * ceil(Ho Wo C/4 / 256) words of scratch)
int launch_bn_relu_maxpool_any(relax_handle* h, const float* x, const float* scale, const float* shift, float* y, void* y_sp3, int Nimg, int H, int W,
                               int C, hipStream_t s, unsigned* amax_out, unsigned* block_ws);
int launch_gap_groups_finish(relax_handle* h, const float* groups, float* out, int Nimg, int HW, int C, int64_t out_stride,
                             hipStream_t s);
int launch_gap_groups_finish_rows(relax_handle* h, const float* groups, float* out, int Nimg, int HW, int C, int64_t out_stride, int group,
                                  hipStream_t s);   // group sums of `group` rows each (gemm_h2.hip's epilogue: 4 at every map size)
int launch_gap(relax_handle* h, const float* x, float* out, int Nimg, int HW, int C, int64_t out_stride,
               hipStream_t s);
// (resnet50.hip) vector v[dim] -> out[0:dim] = v, out[dim .. dim+2] = mean, max, population std; dim = 2048 or 4096
int launch_pool_stats(relax_handle* h, const float* v, int64_t v_stride, float* out, int64_t out_stride, int n, int dim, hipStream_t s);
int launch_nhwc_to_nchw(relax_handle* h, const float* x, float* y, int Nimg, int HW, int C, hipStream_t s);

// model drivers
void free_resnet(relax_handle* h);
void free_vit(relax_handle* h);
void free_resize(relax_handle* h);       // the table cache and resize_ws
void free_head(relax_handle* h);
void free_head_train(relax_handle* h);
void free_vgg(relax_handle* h);
size_t vgg_arena_bytes(int n_images);
size_t resnet_arena_bytes(int n_images, int Hc = 224, int Wc = 224, int flags = 0);   // 0 for a canvas the forward does not take under `flags` (RELAX_RN_CANVAS_ANY)
size_t vit_arena_bytes(const VitW& v, int n_images);                          // at the loaded geometry (224 x 224: relax_reserve)
size_t vit_arena_bytes(const VitW& v, int n_images, int ntok, int npatch);    // at a call's geometry

}  // namespace relax
