// PNG decode on gfx950: relax_png_decode (include/relax_hip.h).  One 64-lane workgroup per image runs the core of
// png_inflate.h with its window ring and Huffman tables in LDS (40 KiB: four images per CU).  See DESIGN.md §8.
#include <hip/hip_runtime.h>

#include "png_inflate.h"
#include "relax_internal.h"

namespace {

__global__ __launch_bounds__(64) void png_decode_kernel(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                        const int64_t* __restrict__ items, uint8_t* out, int64_t out_bytes,
                                                        uint8_t* raw, int64_t raw_bytes, int32_t* status) {
    __shared__ pngd::Shared s;
    const int n = blockIdx.x;
    const int64_t* it = items + (int64_t)n * 8;
    const int64_t so = it[0], sl = it[1], ro = it[2], oo = it[3], H = it[4], W = it[5], C = it[6];
    int st = RELAX_PNG_BAD_ARGS;
    const int64_t rn = (H > 0 && H <= (1 << 24) && W > 0 && W <= pngd::kMaxRowBytes) ? pngd::raw_size(H, W, C) : -1;
    if (rn > 0 && so >= 0 && sl >= 0 && so <= src_bytes && sl <= src_bytes - so && ro >= 0 && ro <= raw_bytes - rn && oo >= 0 &&
        oo <= out_bytes - H * W * 3)
        st = pngd::decode_image(s, src + so, sl, (int)H, (int)W, (int)C, raw + ro, out + oo);
    if (threadIdx.x == 0) status[n] = st;
}

}  // namespace

extern "C" int relax_png_decode(const uint8_t* src, int64_t src_bytes, const int64_t* items, int N, uint8_t* out, int64_t out_bytes,
                                uint8_t* raw, int64_t raw_bytes, int32_t* status, relax_stream stream) {
    if (N < 0 || (N > 0 && (!items || !status || !out || !raw || (!src && src_bytes > 0))) || src_bytes < 0 || out_bytes < 0 ||
        raw_bytes < 0) {
        relax::set_error(nullptr, "relax_png_decode: bad arguments");
        return RELAX_ERR_INVALID;
    }
    if (N == 0) return RELAX_OK;
    png_decode_kernel<<<N, 64, 0, static_cast<hipStream_t>(stream)>>>(src, src_bytes, items, out, out_bytes, raw, raw_bytes, status);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        relax::set_error(nullptr, "relax_png_decode: launch failed: %s", hipGetErrorString(e));
        return RELAX_ERR_HIP;
    }
    return RELAX_OK;
}
