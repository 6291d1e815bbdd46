// Whole-frame front-ends: H x W -> 224 x 224 exactly as Pillow's 8-bit resample does it, for
// the two filters the reference uses:
//   BILINEAR (antialiased)  transforms.Resize((224,224)) on a PIL image   src/extractor/visualise_resnet.py:40-47
//   LANCZOS                 img.resize((224,224), Image.Resampling.LANCZOS) src/extractor/visualise_vit_layer.py:466-469
// Pillow (libImaging/Resample.c): separable, horizontal pass first; coefficients are computed in double, normalised,
// and quantised to 22-bit fixed point; every output is clip8((2^21 + sum(pixel * k)) >> 22); the horizontal result is
// stored as uint8 before the vertical pass.  The coefficient tables are built on the host with the same double
// arithmetic (host::resize_table, which resize_any.hip's any-size kernels share) and cached per (size, filter); the kernels are exact
// integer arithmetic, so the result is bit-identical.
// Each frame is read once (both filters share the horizontal read of a row through LDS).
// relax_resize_residual is the same two passes on the frame difference |next - orig| of a pair (src/main_residual.py:223-231):
// the difference is taken while the rows are staged, so a pair is read once and the residual image itself reaches HBM only when
// the caller asks for it.
#include "relax_internal.h"

namespace relax {

constexpr int OUT = RELAX_TARGET;  // 224
constexpr int PRECISION_BITS = 32 - 8 - 2;
constexpr int ROWS_PER_BLOCK = 4;

__device__ inline uint8_t clip8(int v) {
    v >>= PRECISION_BITS;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

struct ResizeArgs {
    const int32_t* bounds[2];  // per filter
    const int32_t* coeffs[2];
    int ksize[2];
    uint8_t* out[2];           // null = filter not requested
};

// Horizontal pass: a workgroup stages ROWS_PER_BLOCK input rows in LDS (16-byte coalesced loads when aligned) and
// produces the 224 x 3 outputs of both filters for each of them; the coefficient of a tap is loaded once and applied
// to all staged rows.
// PAIR: the staged rows are |next - orig| of a frame pair (`frames` = orig, `next` with the same stride); `residual`
// (contiguous [T,H,W,3], or null) receives the staged bytes.
template <bool PAIR>
__global__ __launch_bounds__(256) void resize_horizontal(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ next,
                                                         int64_t item_stride, int H, int W, ResizeArgs a,
                                                         uint8_t* __restrict__ residual, bool aligned) {
    extern __shared__ __attribute__((aligned(16))) uint8_t rows[];  // [ROWS_PER_BLOCK][row_pad]
    const int n = blockIdx.y;
    const int y0 = blockIdx.x * ROWS_PER_BLOCK;
    const int row_bytes = W * 3;
    const int row_pad = (row_bytes + 15) & ~15;
    const int nrows = H - y0 < ROWS_PER_BLOCK ? H - y0 : ROWS_PER_BLOCK;
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
    if (PAIR && !a.out[0] && !a.out[1]) return;  // residual image only
    __syncthreads();
    for (int o = threadIdx.x; o < 2 * OUT * 3; o += blockDim.x) {
        const int f = o / (OUT * 3);
        if (!a.out[f]) continue;
        const int rem = o - f * OUT * 3;
        const int xx = rem / 3, c = rem - xx * 3;
        const int xmin = a.bounds[f][xx * 2], cnt = a.bounds[f][xx * 2 + 1];
        const int32_t* kk = a.coeffs[f] + (size_t)xx * a.ksize[f];
        int acc[ROWS_PER_BLOCK];
#pragma unroll
        for (int r = 0; r < ROWS_PER_BLOCK; ++r) acc[r] = 1 << (PRECISION_BITS - 1);
        const uint8_t* p = rows + xmin * 3 + c;
        for (int x = 0; x < cnt; ++x) {
            const int k = kk[x];
#pragma unroll
            for (int r = 0; r < ROWS_PER_BLOCK; ++r) acc[r] += (int)p[r * row_pad + x * 3] * k;
        }
        uint8_t* dst = a.out[f] + ((int64_t)n * H + y0) * (OUT * 3) + rem;
#pragma unroll
        for (int r = 0; r < ROWS_PER_BLOCK; ++r)
            if (r < nrows) dst[(int64_t)r * (OUT * 3)] = clip8(acc[r]);
    }
}

// Vertical pass on the uint8 intermediate [N, H, 224, 3] -> [N, 224, 224, 3]; lanes walk adjacent bytes of a row.
__global__ __launch_bounds__(256) void resize_vertical(const uint8_t* __restrict__ tmp, int H, const int32_t* __restrict__ bounds,
                                                       const int32_t* __restrict__ coeffs, int ksize,
                                                       uint8_t* __restrict__ out) {
    const int n = blockIdx.z, yy = blockIdx.y;
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= OUT * 3) return;
    const int ymin = bounds[yy * 2], cnt = bounds[yy * 2 + 1];
    const int32_t* kk = coeffs + (size_t)yy * ksize;
    const uint8_t* p = tmp + ((int64_t)n * H + ymin) * (OUT * 3) + col;
    int acc = 1 << (PRECISION_BITS - 1);
    for (int y = 0; y < cnt; ++y) acc += (int)p[(int64_t)y * (OUT * 3)] * kk[y];
    out[((int64_t)n * OUT + yy) * (OUT * 3) + col] = clip8(acc);
}

static int get_table(relax_handle* h, int in_size, int filt, const ResizeTable** out) {
    for (const ResizeTable& t : h->resize_tables)
        if (t.in_size == in_size && t.filt == filt) {
            *out = &t;
            return RELAX_OK;
        }
    ResizeTable t;
    t.in_size = in_size;
    t.filt = filt;
    t.ksize = host::resize_ksize(in_size, OUT, filt);   // Pillow's precompute_coeffs + normalize_coeffs_8bpc (host_logic.cpp)
    std::vector<int32_t> bounds((size_t)OUT * 2), coeffs((size_t)OUT * t.ksize);
    host::resize_table(in_size, OUT, filt, bounds.data(), coeffs.data());
    RELAX_HIP_CHECK(h, hipMalloc(reinterpret_cast<void**>(&t.bounds), bounds.size() * sizeof(int32_t)));
    RELAX_HIP_CHECK(h, hipMalloc(reinterpret_cast<void**>(&t.coeffs), coeffs.size() * sizeof(int32_t)));
    RELAX_HIP_CHECK(h, hipMemcpy(t.bounds, bounds.data(), bounds.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    RELAX_HIP_CHECK(h, hipMemcpy(t.coeffs, coeffs.data(), coeffs.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    h->resize_tables.push_back(t);
    *out = &h->resize_tables.back();
    return RELAX_OK;
}

void free_resize(relax_handle* h) {
    for (ResizeTable& t : h->resize_tables) {
        (void)hipFree(t.bounds);
        (void)hipFree(t.coeffs);
    }
    h->resize_tables.clear();
    free_resize_any(h);
    if (h->resize_ws.p) (void)hipFree(h->resize_ws.p);
    h->resize_ws = DevBuf();
}

// The two passes behind both entry points: `next` null = plain frames, otherwise |next - frames| per item.
static int run_resize(relax_handle* h, const char* what, const uint8_t* frames, const uint8_t* next, int64_t item_stride, int N, int H,
                      int W, uint8_t* out_bilinear, uint8_t* out_lanczos, uint8_t* residual, relax_stream stream) {
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t* outs[2] = {out_bilinear, out_lanczos};
    const bool any_out = out_bilinear || out_lanczos;
    const int row_pad = (W * 3 + 15) & ~15;
    const size_t lds = (size_t)ROWS_PER_BLOCK * row_pad;
    RELAX_REQUIRE(h, lds <= 64 * 1024, "%s: W=%d too wide for the LDS row stage", what, W);
    // tables first (h->resize_tables may reallocate while growing: fetch every pointer after the last insertion)
    const ResizeTable* t;
    ResizeArgs a{};
    uint8_t* tmp[2] = {nullptr, nullptr};
    if (any_out) {
        for (int f = 0; f < 2; ++f) {
            RELAX_TRY(get_table(h, W, f, &t));
            RELAX_TRY(get_table(h, H, f, &t));
        }
        const size_t tmp_bytes = (size_t)N * H * OUT * 3;
        RELAX_TRY(ensure_buf(h, h->resize_ws, 2 * tmp_bytes));
        tmp[0] = static_cast<uint8_t*>(h->resize_ws.p);
        tmp[1] = tmp[0] + tmp_bytes;
        for (int f = 0; f < 2; ++f) {
            RELAX_TRY(get_table(h, W, f, &t));
            a.bounds[f] = t->bounds;
            a.coeffs[f] = t->coeffs;
            a.ksize[f] = t->ksize;
            a.out[f] = outs[f] ? tmp[f] : nullptr;
        }
    }
    // one switch for loads and the residual store: an odd residual pointer alone sends the call down the bytewise path (relax_hip.h)
    auto at16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    const bool aligned = (W * 3) % 16 == 0 && item_stride % 16 == 0 && at16(frames) && at16(next) && at16(residual);
    const dim3 grid((H + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK, N);
    if (next)
        hipLaunchKernelGGL(resize_horizontal<true>, grid, dim3(256), lds, s, frames, next, item_stride, H, W, a, residual, aligned);
    else
        hipLaunchKernelGGL(resize_horizontal<false>, grid, dim3(256), lds, s, frames, next, item_stride, H, W, a, residual, aligned);
    for (int f = 0; f < 2; ++f) {
        if (!outs[f]) continue;
        RELAX_TRY(get_table(h, H, f, &t));
        hipLaunchKernelGGL(resize_vertical, dim3((OUT * 3 + 255) / 256, OUT, N), dim3(256), 0, s, tmp[f], H, t->bounds,
                           t->coeffs, t->ksize, outs[f]);
    }
    RELAX_HIP_CHECK(h, hipGetLastError());
    return RELAX_OK;
}

}  // namespace relax

using namespace relax;

extern "C" {

int relax_resize_frames(relax_handle* h, const uint8_t* frames, int64_t item_stride, int N, int H, int W,
                        uint8_t* out_bilinear, uint8_t* out_lanczos, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, frames && N > 0 && H > 0 && W > 0, "relax_resize_frames: bad arguments");
    RELAX_REQUIRE(h, out_bilinear || out_lanczos, "relax_resize_frames: no output requested");
    RELAX_REQUIRE(h, item_stride >= (int64_t)H * W * 3 || N == 1, "relax_resize_frames: item stride smaller than a frame");
    return run_resize(h, "relax_resize_frames", frames, nullptr, item_stride, N, H, W, out_bilinear, out_lanczos, nullptr, stream);
}

int relax_resize_residual(relax_handle* h, const uint8_t* orig, const uint8_t* next, int64_t pair_stride, int T, int H, int W,
                          uint8_t* out_bilinear, uint8_t* out_lanczos, uint8_t* residual, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, orig && next && T > 0 && H > 0 && W > 0, "relax_resize_residual: bad arguments");
    RELAX_REQUIRE(h, out_bilinear || out_lanczos || residual, "relax_resize_residual: no output requested");
    RELAX_REQUIRE(h, pair_stride >= (int64_t)H * W * 3 || T == 1, "relax_resize_residual: pair stride smaller than a frame");
    return run_resize(h, "relax_resize_residual", orig, next, pair_stride, T, H, W, out_bilinear, out_lanczos, residual, stream);
}

}  // extern "C"
