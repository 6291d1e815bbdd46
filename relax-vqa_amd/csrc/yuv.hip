// relax_yuv_to_bgr: raw 8-bit planar / NV12 frames -> uint8 HWC BGR (include/relax_hip.h).  Pure streaming: 1.5 bytes per
// pixel in (4:2:0), 3 out.  One lane takes 16 pixels of the rows that share a chroma row; adjacent lanes take adjacent
// 16-byte Y segments, so a wave reads 1 KiB of a Y row per load and writes 3 KiB of an output row with three stores.
// Layout, bounds and arithmetic: yuv_core.h (the same text the CPU tests run).
// relax_yuv_to_bgr_ex: the same lane for the RELAX_YUVF_* formats (2-byte samples, packed rows, chroma shifts up to 2: 1, 2 or 4
// rows per lane), one kernel per kind (sample bytes, packing, hshift, vshift); formats 0..3 go to relax_yuv_to_bgr.
#include <hip/hip_runtime.h>

#include "relax_internal.h"
#include "yuv_core.h"
#include "yuv_load.h"

namespace {

constexpr int kBlock = 256;

// 16 pixels of one row -> 48 bytes, as three 16-byte stores.  cu / cv: the 16 chroma samples of these pixels (replicated
// already), one byte each in four words.
__device__ __forceinline__ void row16(const yuv::Coef& k, const uint4 yq, const uint32_t (&cu)[4], const uint32_t (&cv)[4],
                                      uint8_t* __restrict__ dst) {
    const uint32_t yw[4] = {yq.x, yq.y, yq.z, yq.w};
    uint32_t w[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int p = 0; p < 16; ++p) {
        const int Y = (yw[p >> 2] >> ((p & 3) * 8)) & 255;
        const int U = (cu[p >> 2] >> ((p & 3) * 8)) & 255;
        const int V = (cv[p >> 2] >> ((p & 3) * 8)) & 255;
        int b, g, r;
        yuv::pixel(k, Y, U, V, &b, &g, &r);
        const int i = 3 * p;
        w[i >> 2] |= static_cast<uint32_t>(b) << ((i & 3) * 8);
        w[(i + 1) >> 2] |= static_cast<uint32_t>(g) << (((i + 1) & 3) * 8);
        w[(i + 2) >> 2] |= static_cast<uint32_t>(r) << (((i + 2) & 3) * 8);
    }
    uint4* o = reinterpret_cast<uint4*>(dst);
    o[0] = make_uint4(w[0], w[1], w[2], w[3]);
    o[1] = make_uint4(w[4], w[5], w[6], w[7]);
    o[2] = make_uint4(w[8], w[9], w[10], w[11]);
}

// 8 chroma bytes -> each replicated once: 16 bytes in four words
__device__ __forceinline__ void widen8(const uint2 c, uint32_t (&o)[4]) {
    const uint32_t in[2] = {c.x, c.y};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t h = (in[j >> 1] >> ((j & 1) * 16)) & 0xffffu;   // two samples
        const uint32_t a = h & 255u, b = h >> 8;
        o[j] = a | (a << 8) | (b << 16) | (b << 24);
    }
}

// 16 interleaved bytes U0 V0 U1 V1 ... -> the replicated U and V words
__device__ __forceinline__ void split_nv12(const uint4 c, uint32_t (&u)[4], uint32_t (&v)[4]) {
    const uint32_t in[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t x = in[j];                                       // U a, V a, U b, V b
        const uint32_t ua = x & 255u, va = (x >> 8) & 255u, ub = (x >> 16) & 255u, vb = x >> 24;
        u[j] = ua | (ua << 8) | (ub << 16) | (ub << 24);
        v[j] = va | (va << 8) | (vb << 16) | (vb << 24);
    }
}

__global__ __launch_bounds__(kBlock) void yuv_to_bgr_kernel(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                            const int64_t* __restrict__ items, int layout, int H, int W,
                                                            int matrix, int full_range, uint8_t* __restrict__ out,
                                                            int64_t out_bytes, int32_t* __restrict__ status) {
    const int n = blockIdx.y;
    yuv::Plan p;
    yuv::Coef k;
    if (yuv::plan(layout, H, W, &p) != 0 || !yuv::coef(matrix, full_range, &k)) return;   // refused on the host already
    const int64_t src_off = items[2 * n], out_off = items[2 * n + 1];
    const bool ok = yuv::item_in_range(p, src_off, src_bytes, out_off, out_bytes);
    if (blockIdx.x == 0 && threadIdx.x == 0) status[n] = ok ? RELAX_YUV_OK : RELAX_YUV_OUT_OF_RANGE;
    if (!ok) return;                                                                       // the item writes nothing
    const int64_t unit = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (unit >= yuv::units(p)) return;
    const uint8_t* f = src + src_off;
    uint8_t* o = out + out_off;
    if (!yuv::fast_path(p, reinterpret_cast<uint64_t>(f), reinterpret_cast<uint64_t>(o))) {   // uniform over the block
        yuv::unit_bytewise(p, k, f, o, unit);
        return;
    }
    const yuv::FastUnit a = yuv::fast_unit(p, unit);
    uint32_t cu[4], cv[4];
    if (layout == RELAX_YUV_NV12) {
        split_nv12(*reinterpret_cast<const uint4*>(f + a.u), cu, cv);
    } else if (layout == RELAX_YUV_444P) {
        const uint4 u = *reinterpret_cast<const uint4*>(f + a.u);
        const uint4 v = *reinterpret_cast<const uint4*>(f + a.v);
        cu[0] = u.x, cu[1] = u.y, cu[2] = u.z, cu[3] = u.w;
        cv[0] = v.x, cv[1] = v.y, cv[2] = v.z, cv[3] = v.w;
    } else {
        widen8(*reinterpret_cast<const uint2*>(f + a.u), cu);
        widen8(*reinterpret_cast<const uint2*>(f + a.v), cv);
    }
    const uint4 ya = *reinterpret_cast<const uint4*>(f + a.y[0]);
    uint4 yb = ya;
    if (a.rows == 2) yb = *reinterpret_cast<const uint4*>(f + a.y[1]);   // both loads in flight before the first store
    row16(k, ya, cu, cv, o + a.o[0]);
    if (a.rows == 2) row16(k, yb, cu, cv, o + a.o[1]);
}

// ---- the RELAX_YUVF_* formats -------------------------------------------------------------------------------------------
// 16 pixels of one row -> 48 bytes, as three 16-byte stores
template <class K>
__device__ __forceinline__ void row16_ex(const yuv::Plan& p, const yuv::Coef& k, const uint32_t* lw, const uint32_t* cu,
                                         const uint32_t* cv, uint8_t* __restrict__ dst) {
    uint32_t w[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int px = 0; px < 16; ++px) {
        int b, g, r;
        K::pixel(p, k, lw, cu, cv, px, &b, &g, &r);
        const int i = 3 * px;
        w[i >> 2] |= static_cast<uint32_t>(b) << ((i & 3) * 8);
        w[(i + 1) >> 2] |= static_cast<uint32_t>(g) << (((i + 1) & 3) * 8);
        w[(i + 2) >> 2] |= static_cast<uint32_t>(r) << (((i + 2) & 3) * 8);
    }
    uint4* o = reinterpret_cast<uint4*>(dst);
    o[0] = make_uint4(w[0], w[1], w[2], w[3]);
    o[1] = make_uint4(w[4], w[5], w[6], w[7]);
    o[2] = make_uint4(w[8], w[9], w[10], w[11]);
}

template <int SB, int PACK, int HS, int VS>
__global__ __launch_bounds__(kBlock) void yuv_to_bgr_ex_kernel(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                               const int64_t* __restrict__ items, int format, int H, int W,
                                                               int matrix, int full_range, uint8_t* __restrict__ out,
                                                               int64_t out_bytes, int32_t* __restrict__ status) {
    using K = yuv::Kind<SB, PACK, HS, VS>;
    const int n = blockIdx.y;
    yuv::Plan p;
    yuv::Coef k;
    if (yuv::plan_ex(format, H, W, &p) != 0 || !K::matches(p) || !yuv::coef(matrix, full_range, &k)) return;   // refused on the host already
    const int64_t src_off = items[2 * n], out_off = items[2 * n + 1];
    const bool ok = yuv::item_in_range(p, src_off, src_bytes, out_off, out_bytes);
    if (blockIdx.x == 0 && threadIdx.x == 0) status[n] = ok ? RELAX_YUV_OK : RELAX_YUV_OUT_OF_RANGE;
    if (!ok) return;                                                                       // the item writes nothing
    const int64_t unit = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (unit >= yuv::units_ex(p)) return;
    const uint8_t* f = src + src_off;
    uint8_t* o = out + out_off;
    if (!yuv::fast_path(p, reinterpret_cast<uint64_t>(f), reinterpret_cast<uint64_t>(o))) {   // uniform over the block
        yuv::unit_bytewise_ex(p, k, f, o, unit);
        return;
    }
    const yuv::FastUnitEx a = yuv::fast_unit_ex(p, unit);
    uint32_t lw[K::kRows][K::kYWords], cw[2][K::kCWords];
    if constexpr (K::kCPlanes >= 1) yuv::load_segment<K::kCBytes>(f + a.c[0], cw[0]);
    if constexpr (K::kCPlanes == 2) yuv::load_segment<K::kCBytes>(f + a.c[1], cw[1]);
#pragma unroll
    for (int j = 0; j < K::kRows; ++j)
        if (j < a.rows) yuv::load_segment<K::kYWords * 4>(f + a.y[j], lw[j]);                   // every load in flight before the first store
    const uint32_t* cu = K::kCPlanes == 0 ? lw[0] : cw[0];
    const uint32_t* cv = K::kCPlanes == 0 ? lw[0] : cw[K::kCPlanes == 2 ? 1 : 0];
#pragma unroll
    for (int j = 0; j < K::kRows; ++j)
        if (j < a.rows) row16_ex<K>(p, k, lw[j], cu, cv, o + a.o[j]);
}

// the kernel of a format's kind; formats 0..3 never come here (relax_yuv_to_bgr_ex hands them to yuv_to_bgr_kernel)
using ExKernel = void (*)(const uint8_t*, int64_t, const int64_t*, int, int, int, int, int, uint8_t*, int64_t, int32_t*);
template <int SB, int PACK, int HS, int VS>
struct ExKernelOf {
    static ExKernel get() { return yuv_to_bgr_ex_kernel<SB, PACK, HS, VS>; }
};

}  // namespace

extern "C" int64_t relax_yuv_frame_bytes_ex(int format, int H, int W) {
    yuv::Plan p;
    if (yuv::plan_ex(format, H, W, &p) != 0) return -1;
    return p.frame_bytes;
}

extern "C" int relax_yuv_format_info(int format, int32_t* out) {
    yuv::Format t;
    if (!out || !yuv::format_traits(format, &t)) {
        relax::set_error(nullptr, "relax_yuv_format_info: format %d is not one of RELAX_YUVF_* (0..%d), or out is NULL", format,
                         RELAX_YUVF_COUNT - 1);
        return RELAX_ERR_INVALID;
    }
    out[0] = t.sb, out[1] = t.depth, out[2] = t.shift, out[3] = t.hshift, out[4] = t.vshift, out[5] = t.packing, out[6] = t.swap, out[7] = 0;
    return RELAX_OK;
}

extern "C" int relax_yuv_to_bgr_ex(const uint8_t* src, int64_t src_bytes, const int64_t* items, int N, int format, int H, int W,
                                   int matrix, int full_range, uint8_t* out, int64_t out_bytes, int32_t* status,
                                   relax_stream stream) {
    yuv::Plan p;
    yuv::Coef k;
    const int bad = yuv::plan_ex(format, H, W, &p);
    if (bad == 1) {
        relax::set_error(nullptr, "relax_yuv_to_bgr_ex: format %d is not one of RELAX_YUVF_* (0..%d)", format, RELAX_YUVF_COUNT - 1);
        return RELAX_ERR_INVALID;
    }
    if (bad) {
        relax::set_error(nullptr, "relax_yuv_to_bgr_ex: %s = %d outside 1..%d", bad == 2 ? "H" : "W", bad == 2 ? H : W, yuv::kMaxDim);
        return RELAX_ERR_INVALID;
    }
    if (format <= RELAX_YUVF_NV12)                                 // the 8-bit layouts: relax_yuv_to_bgr's kernel, its checks
        return relax_yuv_to_bgr(src, src_bytes, items, N, format, H, W, matrix, full_range, out, out_bytes, status, stream);
    if (!yuv::coef(matrix, full_range, &k)) {
        relax::set_error(nullptr, "relax_yuv_to_bgr_ex: matrix %d is not RELAX_YUV_BT601 (0) or RELAX_YUV_BT709 (1)", matrix);
        return RELAX_ERR_INVALID;
    }
    if (full_range != 0 && full_range != 1) {
        relax::set_error(nullptr, "relax_yuv_to_bgr_ex: full_range %d is not 0 or 1", full_range);
        return RELAX_ERR_INVALID;
    }
    if (N < 0 || src_bytes < 0 || out_bytes < 0 || (N > 0 && (!items || !status || !out || !src))) {
        relax::set_error(nullptr, "relax_yuv_to_bgr_ex: bad arguments (N %d, src_bytes %lld, out_bytes %lld, or a NULL buffer)", N,
                         static_cast<long long>(src_bytes), static_cast<long long>(out_bytes));
        return RELAX_ERR_INVALID;
    }
    const unsigned blocks = static_cast<unsigned>((yuv::units_ex(p) + kBlock - 1) / kBlock);
    const ExKernel kernel = yuv::for_kind<ExKernelOf, false>(p);
    if (!kernel) {
        relax::set_error(nullptr, "relax_yuv_to_bgr_ex: no kernel for format %d", format);
        return RELAX_ERR_INVALID;
    }
    for (int n0 = 0; n0 < N; n0 += 65535) {                       // gridDim.y holds 65535 items
        const int nn = N - n0 < 65535 ? N - n0 : 65535;
        kernel<<<dim3(blocks, nn), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
            src, src_bytes, items + 2 * static_cast<int64_t>(n0), format, H, W, matrix, full_range, out, out_bytes, status + n0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            relax::set_error(nullptr, "relax_yuv_to_bgr_ex: launch failed: %s", hipGetErrorString(e));
            return RELAX_ERR_HIP;
        }
    }
    return RELAX_OK;
}

extern "C" int64_t relax_yuv_frame_bytes(int layout, int H, int W) {
    yuv::Plan p;
    if (yuv::plan(layout, H, W, &p) != 0) return -1;
    return p.frame_bytes;
}

extern "C" int relax_yuv_coefficients(int matrix, int full_range, int32_t* out) {
    yuv::Coef k;
    if (!out || (full_range != 0 && full_range != 1) || !yuv::coef(matrix, full_range, &k)) {
        relax::set_error(nullptr, "relax_yuv_coefficients: matrix %d / full_range %d refused, or out is NULL", matrix, full_range);
        return RELAX_ERR_INVALID;
    }
    out[0] = k.cy, out[1] = k.oy, out[2] = k.crv, out[3] = k.cbu, out[4] = k.cgu, out[5] = k.cgv;
    return RELAX_OK;
}

extern "C" int relax_yuv_to_bgr(const uint8_t* src, int64_t src_bytes, const int64_t* items, int N, int layout, int H, int W,
                                int matrix, int full_range, uint8_t* out, int64_t out_bytes, int32_t* status,
                                relax_stream stream) {
    yuv::Plan p;
    yuv::Coef k;
    const int bad = yuv::plan(layout, H, W, &p);
    if (bad == 1) {
        relax::set_error(nullptr, "relax_yuv_to_bgr: layout %d is not one of RELAX_YUV_420P/422P/444P/NV12 (0..3)", layout);
        return RELAX_ERR_INVALID;
    }
    if (bad) {
        relax::set_error(nullptr, "relax_yuv_to_bgr: %s = %d outside 1..%d", bad == 2 ? "H" : "W", bad == 2 ? H : W, yuv::kMaxDim);
        return RELAX_ERR_INVALID;
    }
    if (!yuv::coef(matrix, full_range, &k)) {
        relax::set_error(nullptr, "relax_yuv_to_bgr: matrix %d is not RELAX_YUV_BT601 (0) or RELAX_YUV_BT709 (1)", matrix);
        return RELAX_ERR_INVALID;
    }
    if (full_range != 0 && full_range != 1) {
        relax::set_error(nullptr, "relax_yuv_to_bgr: full_range %d is not 0 or 1", full_range);
        return RELAX_ERR_INVALID;
    }
    if (N < 0 || src_bytes < 0 || out_bytes < 0 || (N > 0 && (!items || !status || !out || !src))) {
        relax::set_error(nullptr, "relax_yuv_to_bgr: bad arguments (N %d, src_bytes %lld, out_bytes %lld, or a NULL buffer)", N,
                         static_cast<long long>(src_bytes), static_cast<long long>(out_bytes));
        return RELAX_ERR_INVALID;
    }
    const unsigned blocks = static_cast<unsigned>((yuv::units(p) + kBlock - 1) / kBlock);
    for (int n0 = 0; n0 < N; n0 += 65535) {                       // gridDim.y holds 65535 items
        const int nn = N - n0 < 65535 ? N - n0 : 65535;
        yuv_to_bgr_kernel<<<dim3(blocks, nn), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
            src, src_bytes, items + 2 * static_cast<int64_t>(n0), layout, H, W, matrix, full_range, out, out_bytes, status + n0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            relax::set_error(nullptr, "relax_yuv_to_bgr: launch failed: %s", hipGetErrorString(e));
            return RELAX_ERR_HIP;
        }
    }
    return RELAX_OK;
}
