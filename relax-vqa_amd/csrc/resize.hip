// Whole-frame front-ends: H x W -> out_h x out_w exactly as Pillow's 8-bit resample does it, for the two filters the
// reference uses:
//   BILINEAR (antialiased)  transforms.Resize((224,224)) on a PIL image   src/extractor/visualise_resnet.py:40-47
//   LANCZOS                 img.resize((224,224), Image.Resampling.LANCZOS) src/extractor/visualise_vit_layer.py:466-469
// and, with the size an argument (transforms.Resize(img_size), src/extractor/visualise_vit_layer.py:339-342, the reduced-size form
// commented at :473), for the canvases relax_vit_features_canvas takes.  One kernel family serves every entry: relax_resize_frames and
// relax_resize_residual are the _ex entries at 224 x 224.
// Pillow (libImaging/Resample.c): separable, horizontal pass first, its result stored as uint8, then the vertical pass; a pass whose
// dimension already matches is skipped and the bytes are copied (the intermediate rounding makes order and skips visible).  Coefficients
// are computed in double, normalised and quantised to 22-bit fixed point on the host (host::resize_table) and cached on the device per
// (input size, output size, filter); every output is clip8((2^21 + sum(pixel * k)) >> 22) on an int32 accumulator: exact integer
// arithmetic, so the result is bit-identical.  Each frame is read once (both filters share the horizontal read of a row through LDS).
// The residual entries run the same passes on the frame difference |next - orig| of a pair (src/main_residual.py:223-231): the difference
// is taken while the rows are staged, so a pair is read once and the residual image itself reaches HBM only when the caller asks for it.
// The tap loop: a lane of the horizontal pass owns one output PIXEL of the four staged rows and walks its taps four at a time - one 16-byte
// coefficient load (the device table's rows are padded with zeros to a multiple of four) and, per row, three ALIGNED LDS dword reads whose
// twelve bytes are brought to the lane's byte phase with v_alignbit; products are 24-bit multiply-adds (a byte times a coefficient below
// 2^23); a lane of the vertical pass owns four adjacent bytes of an output row when the rows allow dword access.
#include "relax_internal.h"

namespace relax {
namespace {

static_assert(RELAX_RESIZE_MAX_OUT == host::kResizeMaxOut && RELAX_RESIZE_MAX_IN_H == host::kResizeMaxIn, "relax_hip.h and host_logic.h state the same limits");
static_assert(RELAX_RESIZE_224_MAX_IN_W <= RELAX_RESIZE_MAX_IN_W && RELAX_TARGET <= RELAX_RESIZE_MAX_OUT, "the 224 entries lie inside the kernels' limits");

constexpr int PRECISION_BITS = 32 - 8 - 2;
constexpr int ROWS = 4;         // input rows a workgroup stages
constexpr int LDS_TAIL = 32;    // bytes behind the last staged row: the last group of four taps may reach 16 bytes past the row's end
constexpr int kMaxItems = 65535;   // gridDim.y / .z

__device__ inline uint8_t clip8(int v) {
    v >>= PRECISION_BITS;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// clip8 for a byte that is packed into a dword with others, as clamp-then-shift: hipcc combines the shift-then-clamp form of two packed
// bytes into v_ashr_pk_u8_i32, and on the MI355X the bits above the two bytes of its result were not zero - bytes 2 and 3 of the dword
// came out OR-ed with them (tests/test_gpu_resize_any.py, 18 x 34 -> 48 x 80)
__device__ inline uint32_t clip8_first(int v) {
    v = v < 0 ? 0 : v;
    v = v > (256 << PRECISION_BITS) - 1 ? (256 << PRECISION_BITS) - 1 : v;
    return (uint32_t)v >> PRECISION_BITS;
}

// acc + px * k on the 24-bit multiplier: px is a byte, |k| < 2^23 (any_table checks every coefficient), so the product is exact
__device__ inline int mad24(uint32_t px, int k, int acc) { return __mul24((int)px, k) + acc; }
__device__ inline uint32_t byte_of(uint32_t v, int j) { return (v >> (8 * j)) & 255u; }

struct AnyArgs {
    const int32_t* bounds[2];  // per filter
    const int32_t* coeffs[2];  // rows of kstride ints, 16-byte aligned, zero behind a sample's tap count
    int kstride[2];
    uint8_t* out[2];           // [N, H, out_w, 3] per filter, null = none; copy mode: each non-null one receives the staged bytes
};

// Horizontal pass.  A workgroup stages ROWS input rows in LDS (16-byte loads when `aligned`, bytewise otherwise) and produces the out_w
// pixels of both filters for each of them.
// PAIR: the staged rows are |next - frames| of a pair (same stride); `residual` (contiguous [N,H,W,3], or null) receives them.
// copy (out_w == W, the pass Pillow skips): the staged bytes are the outputs.
template <bool PAIR>
__global__ __launch_bounds__(256) void resize_any_horizontal(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ next,
                                                             int64_t item_stride, int H, int W, int out_w, AnyArgs a,
                                                             uint8_t* __restrict__ residual, bool aligned, bool copy) {
    extern __shared__ __attribute__((aligned(16))) uint8_t rows[];  // [ROWS][row_pad] + LDS_TAIL
    const int n = blockIdx.y;
    const int y0 = blockIdx.x * ROWS;
    const int row_bytes = W * 3;
    const int row_pad = (row_bytes + 15) & ~15;
    const int nrows = H - y0 < ROWS ? H - y0 : ROWS;
    const uint8_t* src = frames + n * item_stride + (int64_t)y0 * row_bytes;
    const uint8_t* src2 = PAIR ? next + n * item_stride + (int64_t)y0 * row_bytes : nullptr;
    uint8_t* res = PAIR && residual ? residual + ((int64_t)n * H + y0) * row_bytes : nullptr;
    if (aligned) {
        const int chunks = row_bytes / 16;
        for (int i = threadIdx.x; i < nrows * chunks; i += blockDim.x) {
            const int r = i / chunks, c = i % chunks;
            uint4 v = *reinterpret_cast<const uint4*>(src + (int64_t)r * row_bytes + c * 16);
            if (PAIR) {
                const uint4 w = *reinterpret_cast<const uint4*>(src2 + (int64_t)r * row_bytes + c * 16);
                v.x = absdiff_u8x4(v.x, w.x);
                v.y = absdiff_u8x4(v.y, w.y);
                v.z = absdiff_u8x4(v.z, w.z);
                v.w = absdiff_u8x4(v.w, w.w);
                if (res) *reinterpret_cast<uint4*>(res + (int64_t)r * row_bytes + c * 16) = v;
            }
            *reinterpret_cast<uint4*>(rows + r * row_pad + c * 16) = v;
        }
    } else {
        for (int i = threadIdx.x; i < nrows * row_bytes; i += blockDim.x) {
            const int r = i / row_bytes, c = i % row_bytes;
            int v = src[(int64_t)r * row_bytes + c];
            if (PAIR) {
                const int w = src2[(int64_t)r * row_bytes + c];
                v = v > w ? v - w : w - v;
                if (res) res[(int64_t)r * row_bytes + c] = (uint8_t)v;
            }
            rows[r * row_pad + c] = (uint8_t)v;
        }
    }
    if (!a.out[0] && !a.out[1]) return;  // residual image only
    __syncthreads();
    if (copy) {
        for (int f = 0; f < 2; ++f) {
            if (!a.out[f]) continue;
            uint8_t* dst = a.out[f] + ((int64_t)n * H + y0) * row_bytes;
            for (int i = threadIdx.x; i < nrows * row_bytes; i += blockDim.x) {
                const int r = i / row_bytes, c = i % row_bytes;
                dst[(int64_t)r * row_bytes + c] = rows[r * row_pad + c];
            }
        }
        return;
    }
    const int out_bytes = out_w * 3;
    for (int o = threadIdx.x; o < 2 * out_w; o += blockDim.x) {
        const int f = o >= out_w ? 1 : 0;
        if (!a.out[f]) continue;
        const int xx = o - f * out_w;
        const int xmin = a.bounds[f][xx * 2], cnt = a.bounds[f][xx * 2 + 1];
        const int4* kq = reinterpret_cast<const int4*>(a.coeffs[f] + (size_t)xx * a.kstride[f]);
        int acc[ROWS][3];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) acc[r][0] = acc[r][1] = acc[r][2] = 1 << (PRECISION_BITS - 1);
        // the taps' bytes start at 3 * xmin: whole dwords from the one that holds that byte, shifted down by the lane's byte phase
        const int b0 = xmin * 3;
        const uint32_t sh = (uint32_t)(b0 & 3) * 8;
        const uint32_t* q = reinterpret_cast<const uint32_t*>(rows) + (b0 >> 2);
        const int rp4 = row_pad >> 2;
        uint32_t w0[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) w0[r] = q[r * rp4];
        const int groups = (cnt + 3) >> 2;   // (bytes behind the last tap meet zero coefficients; rows past nrows hold stale LDS: never stored)
        for (int g = 0; g < groups; ++g) {
            const int4 k = kq[g];
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                const uint32_t* qr = q + r * rp4 + 3 * g;
                const uint32_t w1 = qr[1], w2 = qr[2], w3 = qr[3];
                const uint32_t a0 = __builtin_amdgcn_alignbit(w1, w0[r], sh), a1 = __builtin_amdgcn_alignbit(w2, w1, sh),
                               a2 = __builtin_amdgcn_alignbit(w3, w2, sh);   // twelve bytes = four taps x three channels
                w0[r] = w3;
                acc[r][0] = mad24(byte_of(a0, 0), k.x, acc[r][0]);
                acc[r][1] = mad24(byte_of(a0, 1), k.x, acc[r][1]);
                acc[r][2] = mad24(byte_of(a0, 2), k.x, acc[r][2]);
                acc[r][0] = mad24(byte_of(a0, 3), k.y, acc[r][0]);
                acc[r][1] = mad24(byte_of(a1, 0), k.y, acc[r][1]);
                acc[r][2] = mad24(byte_of(a1, 1), k.y, acc[r][2]);
                acc[r][0] = mad24(byte_of(a1, 2), k.z, acc[r][0]);
                acc[r][1] = mad24(byte_of(a1, 3), k.z, acc[r][1]);
                acc[r][2] = mad24(byte_of(a2, 0), k.z, acc[r][2]);
                acc[r][0] = mad24(byte_of(a2, 1), k.w, acc[r][0]);
                acc[r][1] = mad24(byte_of(a2, 2), k.w, acc[r][1]);
                acc[r][2] = mad24(byte_of(a2, 3), k.w, acc[r][2]);
            }
        }
        uint8_t* dst = a.out[f] + ((int64_t)n * H + y0) * out_bytes + xx * 3;
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
            if (r < nrows) {
                dst[(int64_t)r * out_bytes + 0] = clip8(acc[r][0]);
                dst[(int64_t)r * out_bytes + 1] = clip8(acc[r][1]);
                dst[(int64_t)r * out_bytes + 2] = clip8(acc[r][2]);
            }
    }
}

// Vertical pass on rows of `row_bytes` bytes: item n of `src` at src + n * src_stride, [in_h][row_bytes] -> out [N][out_h][row_bytes].
// VEC: a lane owns four adjacent bytes (dword loads and one dword store; row_bytes, the bases and src_stride are multiples of 4), else one.
template <bool VEC>
__global__ __launch_bounds__(256) void resize_any_vertical(const uint8_t* __restrict__ src, int64_t src_stride, int row_bytes,
                                                           const int32_t* __restrict__ bounds, const int32_t* __restrict__ coeffs, int kstride,
                                                           uint8_t* __restrict__ out, int out_h) {
    const int n = blockIdx.z, yy = blockIdx.y;
    const int col = (blockIdx.x * blockDim.x + threadIdx.x) * (VEC ? 4 : 1);
    if (col >= row_bytes) return;
    const int ymin = bounds[yy * 2], cnt = bounds[yy * 2 + 1];
    const int32_t* kk = coeffs + (size_t)yy * kstride;
    const uint8_t* p = src + n * src_stride + (int64_t)ymin * row_bytes + col;
    uint8_t* dst = out + ((int64_t)n * out_h + yy) * row_bytes + col;
    if (VEC) {
        int acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = 1 << (PRECISION_BITS - 1);
        for (int y = 0; y < cnt; ++y, p += row_bytes) {
            const uint32_t v = *reinterpret_cast<const uint32_t*>(p);
            const int k = kk[y];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = mad24(byte_of(v, j), k, acc[j]);
        }
        *reinterpret_cast<uint32_t*>(dst) =
            clip8_first(acc[0]) | clip8_first(acc[1]) << 8 | clip8_first(acc[2]) << 16 | clip8_first(acc[3]) << 24;
    } else {
        int acc = 1 << (PRECISION_BITS - 1);
        for (int y = 0; y < cnt; ++y, p += row_bytes) acc = mad24(*p, kk[y], acc);
        *dst = clip8(acc);
    }
}

// The cached device table of (in_size, out_size, filt); on a miss the least recently used of the kResizeAnyCache entries is replaced
// (hipFree waits for the device: no launch still reads the table that goes).  One call asks for at most four tables, so the tables it
// fetched earlier are never the ones replaced.
int any_table(relax_handle* h, int in_size, int out_size, int filt, const ResizeAnyTable** out) {
    ResizeAnyTable* slot = &h->resize_any_cache[0];
    for (ResizeAnyTable& t : h->resize_any_cache) {
        if (t.coeffs && t.in_size == in_size && t.out_size == out_size && t.filt == filt) {
            t.used = ++h->resize_any_clock;
            *out = &t;
            return RELAX_OK;
        }
        if (t.used < slot->used) slot = &t;
    }
    // [coeffs out_size x kstride | bounds out_size x 2] in one allocation: the rows of host::resize_table padded with zeros to a multiple of
    // four taps, so a row starts on 16 bytes and a group of four taps never meets a coefficient of the next sample
    const int ksize = host::resize_ksize(in_size, out_size, filt), kstride = (ksize + 3) & ~3;
    std::vector<int32_t> packed((size_t)out_size * ksize), tab((size_t)out_size * (kstride + 2), 0);
    int32_t* bounds = tab.data() + (size_t)out_size * kstride;
    host::resize_table(in_size, out_size, filt, bounds, packed.data());
    for (int i = 0; i < out_size; ++i)
        for (int x = 0; x < ksize; ++x) {
            const int32_t k = packed[(size_t)i * ksize + x];
            RELAX_REQUIRE(h, k > -(1 << 23) && k < (1 << 23), "resize table %d -> %d: coefficient %d outside 24 bits", in_size, out_size, k);
            tab[(size_t)i * kstride + x] = k;
        }
    if (slot->coeffs) {
        RELAX_HIP_CHECK(h, hipFree(slot->coeffs));
        *slot = ResizeAnyTable();
    }
    int32_t* mem = nullptr;
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&mem), tab.size() * sizeof(int32_t));
    if (e != hipSuccess) {
        set_error(h, "hipMalloc of the %d -> %d resize table (%zu bytes) failed: %s", in_size, out_size, tab.size() * sizeof(int32_t),
                  hipGetErrorString(e));
        return RELAX_ERR_NOMEM;
    }
    const hipError_t rc = hipMemcpy(mem, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (rc != hipSuccess) {
        (void)hipFree(mem);
        set_error(h, "upload of the %d -> %d resize table failed: %s", in_size, out_size, hipGetErrorString(rc));
        return RELAX_ERR_HIP;
    }
    slot->in_size = in_size; slot->out_size = out_size; slot->filt = filt; slot->kstride = kstride;
    slot->coeffs = mem; slot->bounds = mem + (size_t)out_size * kstride; slot->used = ++h->resize_any_clock;
    *out = slot;
    return RELAX_OK;
}

// The passes behind both entry points: `next` null = plain frames, otherwise |next - frames| per item.
//   W != out_w, H != out_h : horizontal -> resize_ws [filter][N,H,out_w,3] -> vertical -> outputs
//   W != out_w, H == out_h : horizontal -> outputs
//   W == out_w, H != out_h : vertical straight from the frames; a pair's difference goes through resize_ws first (horizontal in copy mode)
//   W == out_w, H == out_h : horizontal in copy mode -> outputs
int run_resize_any(relax_handle* h, const char* what, const uint8_t* frames, const uint8_t* next, int64_t item_stride, int N, int H, int W,
                   int out_h, int out_w, uint8_t* out_bilinear, uint8_t* out_lanczos, uint8_t* residual, relax_stream stream) {
    RELAX_REQUIRE(h, N <= kMaxItems, "%s: N=%d items, at most %d a call", what, N, kMaxItems);
    RELAX_REQUIRE(h, out_h >= 1 && out_h <= RELAX_RESIZE_MAX_OUT, "%s: out_h=%d outside 1..%d", what, out_h, RELAX_RESIZE_MAX_OUT);
    RELAX_REQUIRE(h, out_w >= 1 && out_w <= RELAX_RESIZE_MAX_OUT, "%s: out_w=%d outside 1..%d", what, out_w, RELAX_RESIZE_MAX_OUT);
    RELAX_REQUIRE(h, H <= RELAX_RESIZE_MAX_IN_H, "%s: H=%d above %d", what, H, RELAX_RESIZE_MAX_IN_H);
    RELAX_REQUIRE(h, W <= RELAX_RESIZE_MAX_IN_W, "%s: W=%d too wide for the LDS row stage (at most %d)", what, W, RELAX_RESIZE_MAX_IN_W);
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t* outs[2] = {out_bilinear, out_lanczos};
    const bool any_out = out_bilinear || out_lanczos;
    const bool hskip = W == out_w, vskip = H == out_h;
    const int row_pad = (W * 3 + 15) & ~15;
    const size_t lds = (size_t)ROWS * row_pad + LDS_TAIL;
    constexpr size_t kWidestLds = (size_t)ROWS * ((RELAX_RESIZE_MAX_IN_W * 3 + 15) & ~15) + LDS_TAIL;
    static_assert(kWidestLds <= (size_t)host::kLdsBytesPerCu, "the widest row stage fits a CU's LDS");
    if (lds > 64 * 1024) {
        static std::atomic<bool> lds_allowed[kMaxDevices];
        RELAX_TRY(allow_dynamic_lds(h, {reinterpret_cast<const void*>(&resize_any_horizontal<false>),
                                        reinterpret_cast<const void*>(&resize_any_horizontal<true>)},
                                    kWidestLds, lds_allowed));
    }
    const ResizeAnyTable* t;
    AnyArgs a{};
    uint8_t* tmp[2] = {nullptr, nullptr};
    const bool run_h = !hskip || vskip || next;   // only the vertical pass of plain frames needs nothing staged
    if (any_out && !vskip && run_h) {
        const size_t tmp_bytes = (size_t)N * H * out_w * 3;
        RELAX_TRY(ensure_buf(h, h->resize_ws, (hskip ? 1 : 2) * tmp_bytes));
        tmp[0] = static_cast<uint8_t*>(h->resize_ws.p);
        tmp[1] = hskip ? tmp[0] : tmp[0] + tmp_bytes;   // the skipped pass's bytes serve both filters
    }
    if (any_out) {
        for (int f = 0; f < 2; ++f) {
            if (!outs[f]) continue;
            if (!hskip) {
                RELAX_TRY(any_table(h, W, out_w, f, &t));
                a.bounds[f] = t->bounds;
                a.coeffs[f] = t->coeffs;
                a.kstride[f] = t->kstride;
            }
            a.out[f] = vskip ? outs[f] : tmp[f];
        }
        if (hskip && !vskip && a.out[0] && a.out[1]) a.out[1] = nullptr;   // one copy of the difference image in resize_ws
    }
    if (run_h) {
        // one switch for loads and the residual store: an odd residual pointer alone sends the call down the bytewise path (relax_hip.h)
        auto at16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
        const bool aligned = (W * 3) % 16 == 0 && item_stride % 16 == 0 && at16(frames) && at16(next) && at16(residual);
        const dim3 grid((H + ROWS - 1) / ROWS, N);
        if (next)
            hipLaunchKernelGGL(resize_any_horizontal<true>, grid, dim3(256), lds, s, frames, next, item_stride, H, W, out_w, a, residual,
                               aligned, hskip);
        else
            hipLaunchKernelGGL(resize_any_horizontal<false>, grid, dim3(256), lds, s, frames, next, item_stride, H, W, out_w, a, residual,
                               aligned, hskip);
    }
    if (!vskip) {
        const int row_bytes = out_w * 3;
        auto at4 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; };
        for (int f = 0; f < 2; ++f) {
            if (!outs[f]) continue;
            RELAX_TRY(any_table(h, H, out_h, f, &t));
            const uint8_t* src = run_h ? tmp[f] : frames;
            const int64_t src_stride = run_h ? (int64_t)H * row_bytes : item_stride;
            const bool vec = row_bytes % 4 == 0 && src_stride % 4 == 0 && at4(src) && at4(outs[f]);
            if (vec)
                hipLaunchKernelGGL(resize_any_vertical<true>, dim3((row_bytes / 4 + 255) / 256, out_h, N), dim3(256), 0, s, src, src_stride,
                                   row_bytes, t->bounds, t->coeffs, t->kstride, outs[f], out_h);
            else
                hipLaunchKernelGGL(resize_any_vertical<false>, dim3((row_bytes + 255) / 256, out_h, N), dim3(256), 0, s, src, src_stride,
                                   row_bytes, t->bounds, t->coeffs, t->kstride, outs[f], out_h);
        }
    }
    RELAX_HIP_CHECK(h, hipGetLastError());
    return RELAX_OK;
}

}  // namespace

void free_resize(relax_handle* h) {
    for (ResizeAnyTable& t : h->resize_any_cache) {
        if (t.coeffs) (void)hipFree(t.coeffs);   // (bounds lives in the same allocation)
        t = ResizeAnyTable();
    }
    if (h->resize_ws.p) (void)hipFree(h->resize_ws.p);
    h->resize_ws = DevBuf();
}

}  // namespace relax

using namespace relax;

extern "C" {

int relax_resize_output_size(int H, int W, int size, int* out_h, int* out_w) {
    std::string err;
    if (!out_h || !out_w) {
        set_error(nullptr, "relax_resize_output_size: out_h or out_w is NULL");
        return RELAX_ERR_INVALID;
    }
    if (!host::resize_output_size(H, W, size, out_h, out_w, err)) {
        set_error(nullptr, "relax_resize_output_size: %s", err.c_str());
        return RELAX_ERR_INVALID;
    }
    return RELAX_OK;
}

int relax_resize_table(int in_size, int out_size, int filt, int32_t* bounds, int32_t* coeffs, int* ksize) {
    const char* bad = nullptr;
    int v = 0;
    if (in_size < 1 || in_size > RELAX_RESIZE_MAX_IN_H) bad = "in_size", v = in_size;
    else if (out_size < 1 || out_size > RELAX_RESIZE_MAX_OUT) bad = "out_size", v = out_size;
    else if (filt != RELAX_RESIZE_BILINEAR && filt != RELAX_RESIZE_LANCZOS) bad = "filt", v = filt;
    if (bad) {
        set_error(nullptr, "relax_resize_table: %s=%d refused (in_size 1..%d, out_size 1..%d, filt 0 = BILINEAR or 1 = LANCZOS)", bad, v,
                  RELAX_RESIZE_MAX_IN_H, RELAX_RESIZE_MAX_OUT);
        return RELAX_ERR_INVALID;
    }
    if (!ksize || (bounds && !coeffs)) {
        set_error(nullptr, "relax_resize_table: ksize is NULL, or bounds without coeffs");
        return RELAX_ERR_INVALID;
    }
    *ksize = host::resize_ksize(in_size, out_size, filt);
    if (bounds) host::resize_table(in_size, out_size, filt, bounds, coeffs);
    return RELAX_OK;
}

// The two 224 x 224 entries: their own argument checks and texts, then run_resize_any at out_h = out_w = 224 (relax_hip.h lists what that
// implies: skipped passes at H or W == 224, the LDS opt-in from W = 5457, N and H refused by name above their limits, the bounded table
// cache).  W stops at RELAX_RESIZE_224_MAX_IN_W, where these entries always stopped.
int relax_resize_frames(relax_handle* h, const uint8_t* frames, int64_t item_stride, int N, int H, int W,
                        uint8_t* out_bilinear, uint8_t* out_lanczos, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, frames && N > 0 && H > 0 && W > 0, "relax_resize_frames: bad arguments");
    RELAX_REQUIRE(h, out_bilinear || out_lanczos, "relax_resize_frames: no output requested");
    RELAX_REQUIRE(h, item_stride >= (int64_t)H * W * 3 || N == 1, "relax_resize_frames: item stride smaller than a frame");
    RELAX_REQUIRE(h, W <= RELAX_RESIZE_224_MAX_IN_W, "relax_resize_frames: W=%d too wide for the LDS row stage (at most %d)", W,
                  RELAX_RESIZE_224_MAX_IN_W);
    return run_resize_any(h, "relax_resize_frames", frames, nullptr, item_stride, N, H, W, RELAX_TARGET, RELAX_TARGET, out_bilinear,
                          out_lanczos, nullptr, stream);
}

int relax_resize_residual(relax_handle* h, const uint8_t* orig, const uint8_t* next, int64_t pair_stride, int T, int H, int W,
                          uint8_t* out_bilinear, uint8_t* out_lanczos, uint8_t* residual, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, orig && next && T > 0 && H > 0 && W > 0, "relax_resize_residual: bad arguments");
    RELAX_REQUIRE(h, out_bilinear || out_lanczos || residual, "relax_resize_residual: no output requested");
    RELAX_REQUIRE(h, pair_stride >= (int64_t)H * W * 3 || T == 1, "relax_resize_residual: pair stride smaller than a frame");
    RELAX_REQUIRE(h, W <= RELAX_RESIZE_224_MAX_IN_W, "relax_resize_residual: W=%d too wide for the LDS row stage (at most %d)", W,
                  RELAX_RESIZE_224_MAX_IN_W);
    return run_resize_any(h, "relax_resize_residual", orig, next, pair_stride, T, H, W, RELAX_TARGET, RELAX_TARGET, out_bilinear,
                          out_lanczos, residual, stream);
}

int relax_resize_frames_ex(relax_handle* h, const uint8_t* frames, int64_t item_stride, int N, int H, int W, int out_h, int out_w,
                           uint8_t* out_bilinear, uint8_t* out_lanczos, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, frames && N > 0 && H > 0 && W > 0, "relax_resize_frames_ex: bad arguments (frames NULL, or N=%d, H=%d, W=%d below 1)", N, H, W);
    RELAX_REQUIRE(h, out_bilinear || out_lanczos, "relax_resize_frames_ex: no output requested (out_bilinear and out_lanczos are NULL)");
    RELAX_REQUIRE(h, item_stride >= (int64_t)H * W * 3 || N == 1, "relax_resize_frames_ex: item stride %lld smaller than a frame",
                  (long long)item_stride);
    return run_resize_any(h, "relax_resize_frames_ex", frames, nullptr, item_stride, N, H, W, out_h, out_w, out_bilinear, out_lanczos, nullptr,
                          stream);
}

int relax_resize_residual_ex(relax_handle* h, const uint8_t* orig, const uint8_t* next, int64_t pair_stride, int T, int H, int W, int out_h,
                             int out_w, uint8_t* out_bilinear, uint8_t* out_lanczos, uint8_t* residual, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, orig && next && T > 0 && H > 0 && W > 0, "relax_resize_residual_ex: bad arguments (orig or next NULL, or T=%d, H=%d, W=%d below 1)",
                  T, H, W);
    RELAX_REQUIRE(h, out_bilinear || out_lanczos || residual, "relax_resize_residual_ex: no output requested");
    RELAX_REQUIRE(h, pair_stride >= (int64_t)H * W * 3 || T == 1, "relax_resize_residual_ex: pair stride %lld smaller than a frame",
                  (long long)pair_stride);
    return run_resize_any(h, "relax_resize_residual_ex", orig, next, pair_stride, T, H, W, out_h, out_w, out_bilinear, out_lanczos, residual,
                          stream);
}

}  // extern "C"
