// The loads of a lane's segments on the 16-byte path of the RELAX_YUVF_* formats (yuv.hip, greyscale.hip): device code only;
// which segment, how wide and where is yuv_core.h's fast_unit_ex.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace yuv {

// NB bytes at an address aligned to min(NB, 16) -> words: one dword, or 16-byte loads
template <int NB>
__device__ __forceinline__ void load_segment(const uint8_t* __restrict__ s, uint32_t* w) {
    if constexpr (NB == 4) {
        w[0] = *reinterpret_cast<const uint32_t*>(s);
    } else if constexpr (NB == 8) {
        const uint2 q = *reinterpret_cast<const uint2*>(s);
        w[0] = q.x, w[1] = q.y;
    } else {
#pragma unroll
        for (int i = 0; i < NB / 16; ++i) {
            const uint4 q = reinterpret_cast<const uint4*>(s)[i];
            w[4 * i] = q.x, w[4 * i + 1] = q.y, w[4 * i + 2] = q.z, w[4 * i + 3] = q.w;
        }
    }
}

}  // namespace yuv
