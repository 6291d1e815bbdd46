// relax_greyscale_scan / relax_yuv_greyscale_scan (include/relax_hip.h): one record of colour-difference maxima per frame.
// Pure streaming reads, 3 bytes per pixel (BGR) or 1.5 (4:2:0), nothing written but 32 bytes per frame.  A lane takes four
// units of 16 pixels, 256 lanes apart, so the 64 lanes of a wave read 3 KiB of adjacent bytes with three 16-byte loads per
// step and all twelve loads of a lane are in flight before its arithmetic starts; then a wave maximum, a block maximum
// through LDS and one atomicMax per block and word on the frame's record (zeroed on the stream before the launch).
// What a lane does with its pixels, and the geometry: greyscale_core.h (the same text the CPU tests run).
// relax_yuv_greyscale_scan_ex: the YUV scan for the RELAX_YUVF_* formats, one kernel per kind as in yuv.hip.
#include <hip/hip_runtime.h>

#include "greyscale_core.h"
#include "relax_internal.h"
#include "yuv_load.h"

namespace {

constexpr int kBlock = grey::kBlock;
constexpr int kLaneUnits = grey::kLaneUnits;
constexpr int kWaves = kBlock / 64;

// every lane of the block arrives here; the record's maxima start at zero and only grow
__device__ __forceinline__ void commit(const grey::Acc& a, int32_t* __restrict__ rec) {
    __shared__ int32_t part[kWaves][6];
    int32_t m[6];
    grey::finish(a, m);
#pragma unroll
    for (int q = 0; q < 6; ++q) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const int32_t o = __shfl_xor(m[q], off, 64);
            m[q] = o > m[q] ? o : m[q];
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 6; ++q) part[threadIdx.x >> 6][q] = m[q];
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        int32_t v = part[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) v = part[w][threadIdx.x] > v ? part[w][threadIdx.x] : v;
        if (v > 0) atomicMax(rec + threadIdx.x, v);
    }
}

__global__ __launch_bounds__(kBlock) void greyscale_scan_kernel(const uint8_t* __restrict__ frames, int64_t frame_stride, int H,
                                                                int W, int32_t* __restrict__ out) {
    const int n = blockIdx.y;
    const uint8_t* f = frames + static_cast<int64_t>(n) * frame_stride;
    const int64_t npix = grey::pixels(H, W), nunits = grey::units(npix);
    grey::Acc a;
    grey::init(&a);
    if (grey::fast_path(reinterpret_cast<uint64_t>(f))) {                                   // uniform over the block
        uint4 q[kLaneUnits][3];
        bool full[kLaneUnits];
#pragma unroll
        for (int j = 0; j < kLaneUnits; ++j) {
            const int64_t unit = grey::unit_of(blockIdx.x, threadIdx.x, j);
            full[j] = grey::unit_is_full(npix, unit);
            if (full[j]) {
                const uint4* s = reinterpret_cast<const uint4*>(f + unit * (grey::kLanePixels * 3));
                q[j][0] = s[0], q[j][1] = s[1], q[j][2] = s[2];
            }
        }
#pragma unroll
        for (int j = 0; j < kLaneUnits; ++j) {
            const int64_t unit = grey::unit_of(blockIdx.x, threadIdx.x, j);
            if (full[j]) {
                const uint32_t w[12] = {q[j][0].x, q[j][0].y, q[j][0].z, q[j][0].w, q[j][1].x, q[j][1].y,
                                        q[j][1].z, q[j][1].w, q[j][2].x, q[j][2].y, q[j][2].z, q[j][2].w};
                grey::unit_words(&a, w);
            } else if (unit < nunits) {
                grey::unit_bytewise(&a, f, npix, unit);                                      // the frame's last, partial unit
            }
        }
    } else {
#pragma unroll 1
        for (int j = 0; j < kLaneUnits; ++j) {
            const int64_t unit = grey::unit_of(blockIdx.x, threadIdx.x, j);
            if (unit < nunits) grey::unit_bytewise(&a, f, npix, unit);
        }
    }
    commit(a, out + static_cast<int64_t>(n) * grey::kRecordWords);
}

// the replicated chroma words of one unit on the 16-byte path
__device__ __forceinline__ void load_chroma(int layout, const uint8_t* __restrict__ f, const yuv::FastUnit& u, uint32_t (&cu)[4],
                                            uint32_t (&cv)[4]) {
    if (layout == RELAX_YUV_NV12) {
        const uint4 c = *reinterpret_cast<const uint4*>(f + u.u);
        const uint32_t in[4] = {c.x, c.y, c.z, c.w};
        grey::split_nv12(in, cu, cv);
    } else if (layout == RELAX_YUV_444P) {
        const uint4 x = *reinterpret_cast<const uint4*>(f + u.u);
        const uint4 y = *reinterpret_cast<const uint4*>(f + u.v);
        cu[0] = x.x, cu[1] = x.y, cu[2] = x.z, cu[3] = x.w;
        cv[0] = y.x, cv[1] = y.y, cv[2] = y.z, cv[3] = y.w;
    } else {
        const uint2 x = *reinterpret_cast<const uint2*>(f + u.u);
        const uint2 y = *reinterpret_cast<const uint2*>(f + u.v);
        const uint32_t xi[2] = {x.x, x.y}, yi[2] = {y.x, y.y};
        grey::widen8(xi, cu);
        grey::widen8(yi, cv);
    }
}

__global__ __launch_bounds__(kBlock) void yuv_greyscale_scan_kernel(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                                    const int64_t* __restrict__ offsets, int layout, int H, int W,
                                                                    int matrix, int full_range, int32_t* __restrict__ out) {
    const int n = blockIdx.y;
    int32_t* rec = out + static_cast<int64_t>(n) * grey::kRecordWords;
    yuv::Plan p;
    yuv::Coef k;
    if (yuv::plan(layout, H, W, &p) != 0 || !yuv::coef(matrix, full_range, &k)) return;    // refused on the host already
    const int64_t src_off = offsets[n];
    const bool ok = grey::yuv_frame_in_range(p, src_off, src_bytes);
    if (!ok) {                                                                              // uniform over the block: nothing is read
        if (blockIdx.x == 0 && threadIdx.x == 0) rec[grey::kStatusWord] = RELAX_YUV_OUT_OF_RANGE;
        return;
    }
    const uint8_t* f = src + src_off;
    const int64_t nunits = yuv::units(p);
    grey::Acc a;
    grey::init(&a);
    if (grey::yuv_fast_path(p, reinterpret_cast<uint64_t>(f))) {                           // uniform over the block
#pragma unroll
        for (int j = 0; j < kLaneUnits; ++j) {
            const int64_t unit = grey::unit_of(blockIdx.x, threadIdx.x, j);
            if (unit < nunits) {
                const yuv::FastUnit u = yuv::fast_unit(p, unit);
                uint32_t cu[4], cv[4];
                load_chroma(layout, f, u, cu, cv);
                const uint4 ya = *reinterpret_cast<const uint4*>(f + u.y[0]);
                uint4 yb = ya;
                if (u.rows == 2) yb = *reinterpret_cast<const uint4*>(f + u.y[1]);
                const uint32_t wa[4] = {ya.x, ya.y, ya.z, ya.w}, wb[4] = {yb.x, yb.y, yb.z, yb.w};
                grey::yuv_row16(&a, k, wa, cu, cv);
                if (u.rows == 2) grey::yuv_row16(&a, k, wb, cu, cv);
            }
        }
    } else {
#pragma unroll 1
        for (int j = 0; j < kLaneUnits; ++j) {
            const int64_t unit = grey::unit_of(blockIdx.x, threadIdx.x, j);
            if (unit < nunits) grey::yuv_unit_bytewise(&a, p, k, f, unit);
        }
    }
    commit(a, rec);
}

// the RELAX_YUVF_* formats: yuv.hip's lane (the segments of yuv::fast_unit_ex, loaded whole before the arithmetic), one unit
// per step, kLaneUnits steps
template <int SB, int PACK, int HS, int VS>
__global__ __launch_bounds__(kBlock) void yuv_greyscale_scan_ex_kernel(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                                       const int64_t* __restrict__ offsets, int format, int H, int W,
                                                                       int matrix, int full_range, int32_t* __restrict__ out) {
    using K = yuv::Kind<SB, PACK, HS, VS>;
    const int n = blockIdx.y;
    int32_t* rec = out + static_cast<int64_t>(n) * grey::kRecordWords;
    yuv::Plan p;
    yuv::Coef k;
    if (yuv::plan_ex(format, H, W, &p) != 0 || !K::matches(p) || !yuv::coef(matrix, full_range, &k)) return;   // refused on the host already
    const int64_t src_off = offsets[n];
    const bool ok = grey::yuv_frame_in_range(p, src_off, src_bytes);
    if (!ok) {                                                                              // uniform over the block: nothing is read
        if (blockIdx.x == 0 && threadIdx.x == 0) rec[grey::kStatusWord] = RELAX_YUV_OUT_OF_RANGE;
        return;
    }
    const uint8_t* f = src + src_off;
    const int64_t nunits = yuv::units_ex(p);
    grey::Acc a;
    grey::init(&a);
    if (grey::yuv_fast_path(p, reinterpret_cast<uint64_t>(f))) {                           // uniform over the block
#pragma unroll
        for (int j = 0; j < kLaneUnits; ++j) {
            const int64_t unit = grey::unit_of(blockIdx.x, threadIdx.x, j);
            if (unit < nunits) {
                const yuv::FastUnitEx u = yuv::fast_unit_ex(p, unit);
                uint32_t lw[K::kRows][K::kYWords], cw[2][K::kCWords];
                if constexpr (K::kCPlanes >= 1) yuv::load_segment<K::kCBytes>(f + u.c[0], cw[0]);
                if constexpr (K::kCPlanes == 2) yuv::load_segment<K::kCBytes>(f + u.c[1], cw[1]);
#pragma unroll
                for (int i = 0; i < K::kRows; ++i)
                    if (i < u.rows) yuv::load_segment<K::kYWords * 4>(f + u.y[i], lw[i]);
                const uint32_t* cu = K::kCPlanes == 0 ? lw[0] : cw[0];
                const uint32_t* cv = K::kCPlanes == 0 ? lw[0] : cw[K::kCPlanes == 2 ? 1 : 0];
#pragma unroll
                for (int i = 0; i < K::kRows; ++i)
                    if (i < u.rows) grey::yuv_row16_ex<K>(&a, p, k, lw[i], cu, cv);
            }
        }
    } else {
#pragma unroll 1
        for (int j = 0; j < kLaneUnits; ++j) {
            const int64_t unit = grey::unit_of(blockIdx.x, threadIdx.x, j);
            if (unit < nunits) grey::yuv_unit_bytewise_ex(&a, p, k, f, unit);
        }
    }
    commit(a, rec);
}

using ExScanKernel = void (*)(const uint8_t*, int64_t, const int64_t*, int, int, int, int, int, int32_t*);
template <int SB, int PACK, int HS, int VS>
struct ExScanKernelOf {
    static ExScanKernel get() { return yuv_greyscale_scan_ex_kernel<SB, PACK, HS, VS>; }
};

int zero_records(const char* who, int32_t* out, int N, hipStream_t stream) {
    const hipError_t e = relax::fill_async(out, 0, static_cast<size_t>(N) * grey::kRecordWords * sizeof(int32_t), stream);
    if (e != hipSuccess) {
        relax::set_error(nullptr, "%s: clearing the records failed: %s", who, hipGetErrorString(e));
        return RELAX_ERR_HIP;
    }
    return RELAX_OK;
}

}  // namespace

extern "C" int relax_greyscale_scan(const uint8_t* frames, int64_t frame_stride, int N, int H, int W, int32_t* out,
                                    relax_stream stream) {
    const int bad = grey::check_size(H, W);
    if (bad) {
        relax::set_error(nullptr, "relax_greyscale_scan: %s = %d outside 1..%d", bad == 1 ? "H" : "W", bad == 1 ? H : W, yuv::kMaxDim);
        return RELAX_ERR_INVALID;
    }
    if (N < 0) {
        relax::set_error(nullptr, "relax_greyscale_scan: N = %d is negative", N);
        return RELAX_ERR_INVALID;
    }
    const int64_t npix = grey::pixels(H, W);
    if (N > 1 && frame_stride < npix * 3) {
        relax::set_error(nullptr, "relax_greyscale_scan: frame_stride = %lld is below the %lld bytes of a %dx%d frame",
                         static_cast<long long>(frame_stride), static_cast<long long>(npix * 3), W, H);
        return RELAX_ERR_INVALID;
    }
    if (N > 0 && (!frames || !out)) {
        relax::set_error(nullptr, "relax_greyscale_scan: %s is NULL with N = %d", !frames ? "frames" : "out", N);
        return RELAX_ERR_INVALID;
    }
    if (N == 0) return RELAX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    RELAX_TRY(zero_records("relax_greyscale_scan", out, N, s));
    const unsigned blocks = static_cast<unsigned>(grey::blocks(grey::units(npix)));
    for (int n0 = 0; n0 < N; n0 += 65535) {                       // gridDim.y holds 65535 frames
        const int nn = N - n0 < 65535 ? N - n0 : 65535;
        greyscale_scan_kernel<<<dim3(blocks, nn), kBlock, 0, s>>>(frames + static_cast<int64_t>(n0) * frame_stride, frame_stride, H, W,
                                                                  out + static_cast<int64_t>(n0) * grey::kRecordWords);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            relax::set_error(nullptr, "relax_greyscale_scan: launch failed: %s", hipGetErrorString(e));
            return RELAX_ERR_HIP;
        }
    }
    return RELAX_OK;
}

extern "C" int relax_yuv_greyscale_scan(const uint8_t* src, int64_t src_bytes, const int64_t* offsets, int N, int layout, int H,
                                        int W, int matrix, int full_range, int32_t* out, relax_stream stream) {
    yuv::Plan p;
    yuv::Coef k;
    const int bad = yuv::plan(layout, H, W, &p);
    if (bad == 1) {
        relax::set_error(nullptr, "relax_yuv_greyscale_scan: layout %d is not one of RELAX_YUV_420P/422P/444P/NV12 (0..3)", layout);
        return RELAX_ERR_INVALID;
    }
    if (bad) {
        relax::set_error(nullptr, "relax_yuv_greyscale_scan: %s = %d outside 1..%d", bad == 2 ? "H" : "W", bad == 2 ? H : W,
                         yuv::kMaxDim);
        return RELAX_ERR_INVALID;
    }
    if (!yuv::coef(matrix, full_range, &k)) {
        relax::set_error(nullptr, "relax_yuv_greyscale_scan: matrix %d is not RELAX_YUV_BT601 (0) or RELAX_YUV_BT709 (1)", matrix);
        return RELAX_ERR_INVALID;
    }
    if (full_range != 0 && full_range != 1) {
        relax::set_error(nullptr, "relax_yuv_greyscale_scan: full_range %d is not 0 or 1", full_range);
        return RELAX_ERR_INVALID;
    }
    if (N < 0 || src_bytes < 0 || (N > 0 && (!offsets || !out || !src))) {
        relax::set_error(nullptr, "relax_yuv_greyscale_scan: bad arguments (N %d, src_bytes %lld, or a NULL buffer)", N,
                         static_cast<long long>(src_bytes));
        return RELAX_ERR_INVALID;
    }
    if (N == 0) return RELAX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    RELAX_TRY(zero_records("relax_yuv_greyscale_scan", out, N, s));
    const unsigned blocks = static_cast<unsigned>(grey::blocks(yuv::units(p)));
    for (int n0 = 0; n0 < N; n0 += 65535) {
        const int nn = N - n0 < 65535 ? N - n0 : 65535;
        yuv_greyscale_scan_kernel<<<dim3(blocks, nn), kBlock, 0, s>>>(src, src_bytes, offsets + n0, layout, H, W, matrix, full_range,
                                                                      out + static_cast<int64_t>(n0) * grey::kRecordWords);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            relax::set_error(nullptr, "relax_yuv_greyscale_scan: launch failed: %s", hipGetErrorString(e));
            return RELAX_ERR_HIP;
        }
    }
    return RELAX_OK;
}

extern "C" int relax_yuv_greyscale_scan_ex(const uint8_t* src, int64_t src_bytes, const int64_t* offsets, int N, int format, int H,
                                           int W, int matrix, int full_range, int32_t* out, relax_stream stream) {
    yuv::Plan p;
    yuv::Coef k;
    const int bad = yuv::plan_ex(format, H, W, &p);
    if (bad == 1) {
        relax::set_error(nullptr, "relax_yuv_greyscale_scan_ex: format %d is not one of RELAX_YUVF_* (0..%d)", format, RELAX_YUVF_COUNT - 1);
        return RELAX_ERR_INVALID;
    }
    if (bad) {
        relax::set_error(nullptr, "relax_yuv_greyscale_scan_ex: %s = %d outside 1..%d", bad == 2 ? "H" : "W", bad == 2 ? H : W,
                         yuv::kMaxDim);
        return RELAX_ERR_INVALID;
    }
    if (format <= RELAX_YUVF_NV12)                                 // the 8-bit layouts: relax_yuv_greyscale_scan's kernel, its checks
        return relax_yuv_greyscale_scan(src, src_bytes, offsets, N, format, H, W, matrix, full_range, out, stream);
    if (!yuv::coef(matrix, full_range, &k)) {
        relax::set_error(nullptr, "relax_yuv_greyscale_scan_ex: matrix %d is not RELAX_YUV_BT601 (0) or RELAX_YUV_BT709 (1)", matrix);
        return RELAX_ERR_INVALID;
    }
    if (full_range != 0 && full_range != 1) {
        relax::set_error(nullptr, "relax_yuv_greyscale_scan_ex: full_range %d is not 0 or 1", full_range);
        return RELAX_ERR_INVALID;
    }
    if (N < 0 || src_bytes < 0 || (N > 0 && (!offsets || !out || !src))) {
        relax::set_error(nullptr, "relax_yuv_greyscale_scan_ex: bad arguments (N %d, src_bytes %lld, or a NULL buffer)", N,
                         static_cast<long long>(src_bytes));
        return RELAX_ERR_INVALID;
    }
    if (N == 0) return RELAX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    RELAX_TRY(zero_records("relax_yuv_greyscale_scan_ex", out, N, s));
    const unsigned blocks = static_cast<unsigned>(grey::blocks(yuv::units_ex(p)));
    const ExScanKernel kernel = yuv::for_kind<ExScanKernelOf, false>(p);
    if (!kernel) {
        relax::set_error(nullptr, "relax_yuv_greyscale_scan_ex: no kernel for format %d", format);
        return RELAX_ERR_INVALID;
    }
    for (int n0 = 0; n0 < N; n0 += 65535) {
        const int nn = N - n0 < 65535 ? N - n0 : 65535;
        kernel<<<dim3(blocks, nn), kBlock, 0, s>>>(src, src_bytes, offsets + n0, format, H, W, matrix, full_range,
                                                   out + static_cast<int64_t>(n0) * grey::kRecordWords);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            relax::set_error(nullptr, "relax_yuv_greyscale_scan_ex: launch failed: %s", hipGetErrorString(e));
            return RELAX_ERR_HIP;
        }
    }
    return RELAX_OK;
}
