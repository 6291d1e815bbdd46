// The decode core of png_inflate.h as plain host C++ (one lane), with exactly sized heap buffers: built alone under
// AddressSanitizer + UBSan (make sanitize_png) and driven by tests/png_decode_driver.py.  Not part of librelax_hip.so.
#include <cstdlib>
#include <vector>

#include "png_inflate.h"

extern "C" int relax_png_decode_host(const uint8_t* z, int64_t zlen, int H, int W, int C, uint8_t* out, int64_t out_bytes) {
    const int64_t n = pngd::raw_size(H, W, C);
    if (n < 0 || !out || zlen < 0 || out_bytes < (int64_t)H * W * 3) return RELAX_PNG_BAD_ARGS;
    std::vector<uint8_t> raw((size_t)n);
    pngd::Shared* s = new pngd::Shared;
    const int st = pngd::decode_image(*s, z, zlen, H, W, C, raw.data(), out);
    delete s;
    return st;
}
