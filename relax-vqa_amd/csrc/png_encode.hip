// PNG encode on gfx950: relax_png_encode (include/relax_hip.h).  Four launches per call run the core of png_deflate.h:
// the plan (one workgroup: items -> bands and their scratch slots), the bands (one 256-thread workgroup per band, the
// filtered bytes and the output bits in LDS; a fixed grid walks the bands of all images), the placement (one workgroup
// per image: prefix sums of the band lengths, zlib header, combined Adler-32, length and status) and the copy of every
// band to its place.  See DESIGN.md section 8.
#include <hip/hip_runtime.h>

#include "png_deflate.h"
#include "relax_internal.h"

namespace {

constexpr int kGrid = 1024;     // workgroups of the band kernels: each walks the bands g, g + kGrid, ...

__global__ __launch_bounds__(pnge::kThreads) void png_plan_kernel(const int64_t* __restrict__ items, int N, int64_t images_bytes,
                                                                  int64_t out_bytes, uint8_t* scratch, int64_t scratch_bytes,
                                                                  int64_t* lengths, int32_t* status) {
    __shared__ uint64_t tmp[pnge::kThreads];
    pnge::plan(tmp, items, N, images_bytes, out_bytes, scratch, scratch_bytes, lengths, status);
}

__global__ __launch_bounds__(pnge::kThreads) void png_encode_kernel(const uint8_t* __restrict__ images,
                                                                    const int64_t* __restrict__ items, int N, uint8_t* scratch) {
    __shared__ pnge::Shared s;
    const int64_t total = *(const int64_t*)scratch;
    for (int64_t g = blockIdx.x; g < total; g += gridDim.x) pnge::encode_band(s, images, items, N, scratch, g);
}

__global__ __launch_bounds__(pnge::kThreads) void png_place_kernel(const int64_t* __restrict__ items, int N, uint8_t* out,
                                                                   uint8_t* scratch, int64_t* lengths, int32_t* status) {
    __shared__ uint64_t tmp[pnge::kThreads];
    pnge::place_bands(tmp, items, N, blockIdx.x, out, scratch, lengths, status);
}

__global__ __launch_bounds__(pnge::kThreads) void png_copy_kernel(const int64_t* __restrict__ items, int N, uint8_t* out,
                                                                  const uint8_t* scratch) {
    const int64_t total = *(const int64_t*)scratch;
    for (int64_t g = blockIdx.x; g < total; g += gridDim.x) pnge::copy_band(items, N, out, scratch, g);
}

}  // namespace

extern "C" int64_t relax_png_encode_bound(int H, int W, int C, int filter, int64_t* scratch_bytes, int* band_rows) {
    int64_t scratch = 0, rows = 0;
    const int64_t b = pnge::bound(H, W, C, filter, &scratch, &rows, nullptr, nullptr);
    if (b < 0) return -1;
    if (scratch_bytes) *scratch_bytes = scratch;
    if (band_rows) *band_rows = (int)rows;
    return b;
}

extern "C" int relax_png_encode_passes(const uint8_t* images, int64_t images_bytes, const int64_t* items, int N, uint8_t* out,
                                       int64_t out_bytes, uint8_t* scratch, int64_t scratch_bytes, int64_t* lengths,
                                       int32_t* status, int passes, relax_stream stream) {
    if (N < 0 || images_bytes < 0 || out_bytes < 0 || scratch_bytes < 0 || passes < 0 || passes > RELAX_PNG_ENCODE_ALL ||
        (N > 0 && (!items || !images || !out || !scratch || !lengths || !status || ((uintptr_t)scratch & 7) ||
                   scratch_bytes < pnge::kPlanHeader + (int64_t)pnge::kPlanEntry * N))) {
        relax::set_error(nullptr, "relax_png_encode: bad arguments");
        return RELAX_ERR_INVALID;
    }
    if (N == 0) return RELAX_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (passes & RELAX_PNG_ENCODE_PLAN)
        png_plan_kernel<<<1, pnge::kThreads, 0, st>>>(items, N, images_bytes, out_bytes, scratch, scratch_bytes, lengths, status);
    if (passes & RELAX_PNG_ENCODE_BANDS) png_encode_kernel<<<kGrid, pnge::kThreads, 0, st>>>(images, items, N, scratch);
    if (passes & RELAX_PNG_ENCODE_PLACE) png_place_kernel<<<N, pnge::kThreads, 0, st>>>(items, N, out, scratch, lengths, status);
    if (passes & RELAX_PNG_ENCODE_COPY) png_copy_kernel<<<kGrid, pnge::kThreads, 0, st>>>(items, N, out, scratch);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        relax::set_error(nullptr, "relax_png_encode: launch failed: %s", hipGetErrorString(e));
        return RELAX_ERR_HIP;
    }
    return RELAX_OK;
}

extern "C" int relax_png_encode(const uint8_t* images, int64_t images_bytes, const int64_t* items, int N, uint8_t* out,
                                int64_t out_bytes, uint8_t* scratch, int64_t scratch_bytes, int64_t* lengths, int32_t* status,
                                relax_stream stream) {
    return relax_png_encode_passes(images, images_bytes, items, N, out, out_bytes, scratch, scratch_bytes, lengths, status,
                                   RELAX_PNG_ENCODE_ALL, stream);
}
