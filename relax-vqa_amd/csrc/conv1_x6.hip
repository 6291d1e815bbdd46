// ResNet-50 conv1 (7x7, stride 2, pad 3, 3 -> 64 channels, no bias: the raw pre-BN tap) under "bf16x6", straight from the uint8
// fragments: ToTensor + Normalize, im2col, the split into bf16 planes and the contraction in one kernel.
//
// The generic implicit-GEMM kernel (gemm_x6.hip) wants 16-channel chunks per tap; with 3 input channels that would be 49 taps x 16 =
// 5.3x the MACs.  Here the K axis is (ky, kx, c) with the 7 x 3 = 21 values of one filter row padded to 32 (two 16-deep MFMA steps):
// K = 7 x 32 = 224 against 147 real - 9.1 bf16 MFMA passes per fp32 MAC instead of the 16 of the exact-fp32 kernel that ran this
// layer before (3.7 ms per 1024 fragments, 1.5 % of a config-3 step).  The 21 values of a (pixel, ky) are CONTIGUOUS in an RGB-interleaved
// image row, so an MFMA A fragment (8 consecutive k of one output pixel) is 8 consecutive floats of the input patch:
//   * a persistent workgroup (8 waves) keeps the 64 x 224 weights as split planes in LDS (85 KB) and walks 256-pixel tiles of the
//     112x112 output (49 per image: a tile never straddles two images);
//   * per tile it normalises the up to 13 input rows the tile's pixels tap into an fp32 patch in LDS (zero padded borders); the patch
//     is double-buffered: the next tile's rows are requested (as dwords, into registers) before the MFMA loop and written after it,
//   * every wave owns 32 output pixels x 64 channels: per K step it reads its 8 patch floats per lane, splits them into hi / mid / lo
//     (exact), reads the weight fragments and issues the six partial products (smallest first, as gemm_x6);
//   * the accumulators go straight to the NHWC fp32 output (a register of a 32x32 tile is 32 consecutive channels of one pixel),
//     and the 16-pixel group sums of the fused spatial mean (tap 0 of the layer stack) are formed in registers.
// Columns 21 .. 31 of a padded filter row read whatever follows in the patch (finite values) against ZERO weights.
// H2 ("f16x2", with "rn_h2_early"): the same kernel on two fp16 planes - the patch values x 2^13 (|normalised pixel| <= 2.64: a static
// scale) split in registers, the weights as planes with one power-of-two scale per filter, the three partial products al bh, ah bl, ah bh
// on v_mfma_f32_32x32x16_f16 with the two small ones in accumulators of their own (gemm_x6.hip, H2), half the matrix instructions.
#include "relax_internal.h"
#include "sp3.h"
#include "h2.h"

namespace relax {

typedef float c1_floatx16 __attribute__((ext_vector_type(16)));
typedef __bf16 c1_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 c1_f16x8 __attribute__((ext_vector_type(8)));
[[maybe_unused]] constexpr float kC1PatchScale = 8192.f;   // H2: 2.64 * 2^13 = 21.6 k < 65504
typedef float c1_f32x2 __attribute__((ext_vector_type(2)));

constexpr int C1_HW = 224, C1_OW = 112, C1_OPIX = C1_OW * C1_OW;   // 12544 = 49 * 256
constexpr int C1_TILE = 256;
constexpr int C1_KROW = 32;                         // 21 real (kx, c) values per filter row, padded
constexpr int C1_K = 7 * C1_KROW;                   // 224
constexpr int C1_CHUNKS = C1_K / 16;                // 14
constexpr int C1_WROW = C1_CHUNKS * kChunkBytes + 16;   // LDS bytes per weight row (+16: conflict-free ds_read_b128 across rows)
constexpr int C1_PCOLS = (C1_HW + 6) * 3;           // 690 floats per patch row (3 padding pixels on each side)
constexpr int C1_PROW = C1_PCOLS + 2;               // 692 (even: 8-byte aligned fragment reads)
constexpr int C1_PROWS = 13;                        // 2 * 3 + 7: a tile spans at most 4 output rows
constexpr int C1_W_BYTES = 64 * C1_WROW;
constexpr int C1_PATCH_FLOATS = C1_PROWS * C1_PROW + 64;   // slack: the padded k columns of the last row read past its end
constexpr size_t C1_LDS = C1_W_BYTES + 2 * sizeof(float) * C1_PATCH_FLOATS + 3 * 256 * sizeof(float);   // weights + two patch buffers + the normalisation table: 158.8 of 160 KiB

// fp32 weights [64][Kpad] of the exact-fp32 kernel, k = (ky*7 + kx)*4 + c  ->  [64][224], k = ky*32 + kx*3 + c (zeros elsewhere)
__global__ __launch_bounds__(256) void conv1_repack(const float* __restrict__ w, int kpad, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 64 * C1_K) return;
    const int n = i / C1_K, k = i - n * C1_K;
    const int ky = k / C1_KROW, j = k - ky * C1_KROW;
    float v = 0.f;
    if (j < 21) v = w[(int64_t)n * kpad + (ky * 7 + j / 3) * 4 + j % 3];
    out[i] = v;
}

// one dword = 4 consecutive bytes k = 4d .. 4d+3 of a 672-byte BGR image row -> normalised RGB floats at their patch positions
// (k = 3 px + c, c: 0 = B, 1 = G, 2 = R  ->  patch column 9 + 3 px + (2 - c) = 11 + k - 2c).  lut[c][byte] = ((byte / 255) - mean_c) /
// std_c, computed once per workgroup with the operations of rn_preprocess (two fp32 divisions per value are ~25 instructions:
// looked up, not redone 20 times per thread and tile)
__device__ inline void conv1_put4(float* prow, int d, unsigned v, bool valid, const float* lut) {
    const int d3 = d % 3;                                  // 4d mod 3
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int c = (d3 + b) % 3;
        prow[11 + 4 * d + b - 2 * c] = valid ? lut[c * 256 + ((v >> (8 * b)) & 255u)] : 0.f;   // zeros above / below the image
    }
}

constexpr int C1_ROW_DW = C1_HW * 3 / 4;                   // 168 dwords per image row
[[maybe_unused]] constexpr int C1_LOADS = (C1_PROWS * C1_ROW_DW + 511) / 512;   // 5 dwords per thread and tile

template <bool H2>
__global__ __launch_bounds__(512) void conv1_x6(const uint8_t* __restrict__ frags, const char* __restrict__ w_sp3, float* __restrict__ out,
                                                float* __restrict__ gap, int n_tiles, const float* __restrict__ w_inv) {
#if __HIP_DEVICE_COMPILE__
    constexpr int CH = H2 ? kH2ChunkBytes : kChunkBytes;          // bytes of a 16-deep chunk of a weight row (two fp16 / three bf16 planes)
    constexpr int UPR = C1_CHUNKS * CH / 16;                      // 16-byte units per weight row
    constexpr int WROW = C1_CHUNKS * CH + 16;                     // (+16: conflict-free ds_read_b128 across rows, both forms)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* wl = smem;
    float* patch0 = reinterpret_cast<float*>(smem + C1_W_BYTES);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, half = lane >> 5;

    // weights: 64 rows x 84 16-byte units, rows padded to C1_WROW bytes; both patch buffers start as zeros (their 3-pixel side
    // borders and the slack are never written again)
    for (int u = tid; u < 64 * UPR; u += 512) {
        const int n = u / UPR, q = u - n * UPR;
        *reinterpret_cast<sp3_u32x4*>(wl + n * WROW + q * 16) = *reinterpret_cast<const sp3_u32x4*>(w_sp3 + ((int64_t)n * UPR + q) * 16);
    }
    for (int i = tid; i < 2 * C1_PATCH_FLOATS; i += 512) patch0[i] = 0.f;
    float* lut = patch0 + 2 * C1_PATCH_FLOATS;
    for (int i = tid; i < 3 * 256; i += 512) {
        const int c = i >> 8;
        const float u = (float)(i & 255) / 255.0f;                                                      // as rn_preprocess
        lut[i] = c == 2 ? (u - 0.485f) / 0.229f : c == 1 ? (u - 0.456f) / 0.224f : (u - 0.406f) / 0.225f;
    }
    __syncthreads();

    // the input rows of a tile as raw dwords in registers (requested before the MFMA loop of the tile before, written after it)
    unsigned raw[C1_LOADS];
    auto tile_geom = [&](int t, int& img, int& p0, int& y0, int& iy0, int& rows) {
        img = t / (C1_OPIX / C1_TILE);
        p0 = (t - img * (C1_OPIX / C1_TILE)) * C1_TILE;
        y0 = p0 / C1_OW;
        iy0 = 2 * y0 - 3;
        rows = 2 * ((p0 + C1_TILE - 1) / C1_OW - y0) + 7;
    };
    auto request = [&](int t) {
        int img, p0, y0, iy0, rows;
        tile_geom(t, img, p0, y0, iy0, rows);
        const unsigned* im = reinterpret_cast<const unsigned*>(frags + (int64_t)img * (C1_HW * C1_HW * 3));
#pragma unroll
        for (int i = 0; i < C1_LOADS; ++i) {
            const int e = tid + 512 * i;
            const int row = e / C1_ROW_DW, d = e - row * C1_ROW_DW;
            const int iy = iy0 + row;
            raw[i] = (row < rows && (unsigned)iy < (unsigned)C1_HW) ? im[iy * C1_ROW_DW + d] : 0u;
        }
    };
    auto deposit = [&](int t, float* patch) {
        int img, p0, y0, iy0, rows;
        tile_geom(t, img, p0, y0, iy0, rows);
#pragma unroll
        for (int i = 0; i < C1_LOADS; ++i) {
            const int e = tid + 512 * i;
            const int row = e / C1_ROW_DW, d = e - row * C1_ROW_DW;
            if (row < rows) conv1_put4(patch + row * C1_PROW, d, raw[i], (unsigned)(iy0 + row) < (unsigned)C1_HW, lut);
        }
    };

    int cur = 0;
    if ((int)blockIdx.x < n_tiles) {
        request(blockIdx.x);
        deposit(blockIdx.x, patch0);
    }
    __syncthreads();
    for (int t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        int img, p0, y0, iy0, rows;
        tile_geom(t, img, p0, y0, iy0, rows);
        const float* patch = patch0 + cur * C1_PATCH_FLOATS;
        const int next = t + gridDim.x;
        if (next < n_tiles) request(next);                 // in flight under the MFMAs below

        const int p = p0 + wave * 32 + r;                  // this lane's output pixel (A rows of the wave's 32x64 block)
        const int y = p / C1_OW, x = p - y * C1_OW;
        const float* arow = patch + (2 * (y - y0)) * C1_PROW + 6 * x + 8 * half;
        c1_floatx16 acc[2], accs[2];   // (accs: H2's small products)
#pragma unroll
        for (int i = 0; i < 16; ++i) { acc[0][i] = 0.f; acc[1][i] = 0.f; accs[0][i] = 0.f; accs[1][i] = 0.f; }
#pragma unroll
        for (int ky = 0; ky < 7; ++ky) {
#pragma unroll
            for (int jc = 0; jc < 2; ++jc) {
                const float* a = arow + ky * C1_PROW + 16 * jc;
                const c1_f32x2 a0 = *reinterpret_cast<const c1_f32x2*>(a), a1 = *reinterpret_cast<const c1_f32x2*>(a + 2),
                               a2 = *reinterpret_cast<const c1_f32x2*>(a + 4), a3 = *reinterpret_cast<const c1_f32x2*>(a + 6);
                const int chunk = ky * 2 + jc;
                if constexpr (H2) {
                    h2_u32x4 ah, al;
                    split2_x8((h2_f32x4){a0.x, a0.y, a1.x, a1.y} * kC1PatchScale, (h2_f32x4){a2.x, a2.y, a3.x, a3.y} * kC1PatchScale, ah, al);
                    const c1_f16x8 Ah = __builtin_bit_cast(c1_f16x8, ah), Al = __builtin_bit_cast(c1_f16x8, al);
                    c1_f16x8 Bh[2], Bl[2];
#pragma unroll
                    for (int cb = 0; cb < 2; ++cb) {
                        const char* wp = wl + (cb * 32 + r) * WROW + chunk * CH + half * 16;
                        Bh[cb] = *reinterpret_cast<const c1_f16x8*>(wp);
                        Bl[cb] = *reinterpret_cast<const c1_f16x8*>(wp + 32);
                    }
                    accs[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Al, Bh[0], accs[0], 0, 0, 0);
                    accs[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Al, Bh[1], accs[1], 0, 0, 0);
                    accs[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Bl[0], accs[0], 0, 0, 0);
                    accs[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Bl[1], accs[1], 0, 0, 0);
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Bh[0], acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Bh[1], acc[1], 0, 0, 0);
                    continue;
                }
                sp3_u32x4 ah, am, al;
                split3_x8((sp3_f32x4){a0.x, a0.y, a1.x, a1.y}, (sp3_f32x4){a2.x, a2.y, a3.x, a3.y}, ah, am, al);
                const c1_bf16x8 Ah = __builtin_bit_cast(c1_bf16x8, ah), Am = __builtin_bit_cast(c1_bf16x8, am),
                                Al = __builtin_bit_cast(c1_bf16x8, al);
                c1_bf16x8 Bh[2], Bm[2], Bl[2];
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) {
                    const char* wp = wl + (cb * 32 + r) * WROW + chunk * CH + half * 16;
                    Bh[cb] = *reinterpret_cast<const c1_bf16x8*>(wp);
                    Bm[cb] = *reinterpret_cast<const c1_bf16x8*>(wp + 32);
                    Bl[cb] = *reinterpret_cast<const c1_bf16x8*>(wp + 64);
                }
                // the six partial products, smallest first; the two accumulators alternate (no MFMA waits on the one before it)
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Al, Bh[0], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Al, Bh[1], acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Am, Bm[0], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Am, Bm[1], acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bl[0], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bl[1], acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Am, Bh[0], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Am, Bh[1], acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bm[0], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bm[1], acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bh[0], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bh[1], acc[1], 0, 0, 0);
            }
        }
        // acc[cb][i]: channel cb*32 + r of pixel  32*wave + (i & 3) + 8 * (i >> 2) + 4 * half
        const int64_t pix0 = (int64_t)img * C1_OPIX + p0 + wave * 32;
        if constexpr (H2) {   // the scales are powers of two: exact
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) acc[cb] = (acc[cb] + accs[cb]) * (w_inv[cb * 32 + r] * (1.f / kC1PatchScale));
        }
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
#pragma unroll
            for (int i = 0; i < 16; ++i)
                out[(pix0 + (i & 3) + 8 * (i >> 2) + 4 * half) * 64 + cb * 32 + r] = acc[cb][i];
            if (gap) {   // sums over the two aligned groups of 16 pixels of this wave (pixels in a fixed order: batch-invariant)
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    float s = 0.f;
#pragma unroll
                    for (int i = 0; i < 8; ++i) s += acc[cb][8 * g + i];
                    s += __shfl_xor(s, 32);
                    if (half == 0) gap[((pix0 >> 4) + g) * 64 + cb * 32 + r] = s;
                }
            }
        }
        if (next < n_tiles) deposit(next, patch0 + (cur ^ 1) * C1_PATCH_FLOATS);   // the other buffer: nobody reads it during this tile
        __syncthreads();                                   // next patch complete, every wave done with this one
        cur ^= 1;
    }
#endif
}

// ---- the same stem on any accepted canvas (Hc, Wc multiples of 32: host_logic.h, rn_canvas_geometry) -------------------------------------------
// Geometry at run time.  conv1_x6 above walks 256 CONSECUTIVE output pixels and keeps their up to 13 input rows at full width: 18 KB per patch
// at 224, but 3 output rows of a 288-wide canvas already take 39 KB and half a row of a 1024-wide one 87 KB - two of them do not fit beside
// the 85 KB of weights.  Here a tile is 16 x 16 output pixels: the output maps are multiples of 16 both ways, so a tile never straddles two
// images, there are (Hc / 2) (Wc / 2) / 256 per image as before, and its 16 rows of 16 pixels ARE the aligned 16-pixel groups of the fused
// spatial mean (16 consecutive pixels never cross a row end).  Its patch is 37 rows x 37 pixels on every canvas (19 KB): a wave owns two of the
// tile's rows, the K loop, the split and the order of the products are conv1_x6's (conv1_mma below restates its loop; the 224 kernel keeps its
// own copy so that its code stays as it was) - every output value and every group sum has the bits the 224 kernel gives it.
// A patch row is the 29 dwords that cover pixels 2 x0 - 4 .. 2 x0 + 34 of an image row (x0 a multiple of 16: byte 96 k - 12, dword-aligned
// and a multiple of 3); dwords left or right of the image and rows above or below it are deposited as zeros, so every tile rewrites its whole
// window and nothing depends on the tile that used the buffer before.
constexpr int C1C_T = 16;                                  // tile side in output pixels
constexpr int C1C_PROWS = 2 * (C1C_T - 1) + 7;             // 37 input rows
constexpr int C1C_ROW_DW = 29;                             // dwords per patch row: bytes -12 .. 104 of the window (pixels -4 .. 34 + 2 bytes)
constexpr int C1C_COL0 = 4;                                // patch column of pixel 2 x0 - 3, channel R (even: 8-byte aligned fragment reads)
constexpr int C1C_PROW = 130;                              // floats per patch row: 3 + 116 deposited, the padded k columns of the last pixel read up to 125
constexpr int C1C_PATCH_FLOATS = C1C_PROWS * C1C_PROW + 64;
[[maybe_unused]] constexpr int C1C_LOADS = (C1C_PROWS * C1C_ROW_DW + 511) / 512;   // 3 dwords per thread and tile
constexpr size_t C1C_LDS = C1_W_BYTES + 2 * sizeof(float) * C1C_PATCH_FLOATS + 3 * 256 * sizeof(float);   // 126.4 KiB
static_assert(C1C_COL0 + 6 * (C1C_T - 1) + 8 + 16 + 8 <= C1C_PROW && C1C_PROW % 2 == 0 && C1C_PATCH_FLOATS % 2 == 0, "the last lane's fragment stays inside its patch row");
static_assert(4 * (C1C_ROW_DW - 1) + 3 + 3 < C1C_PROW, "every deposited byte lands inside its patch row");

// dword d of a patch row's window (bytes 4 d .. 4 d + 3 from byte 96 k - 12 of a BGR image row, channel (d + b) % 3) -> patch columns
// C1C_COL0 + 3 (px - (2 x0 - 3)) + (2 - c) = 4 d + b + 3 - 2 c   (>= 1: column 0 and the columns behind 118 stay the zeros they start as)
__device__ inline void conv1_canvas_put4(float* prow, int d, unsigned v, bool valid, const float* lut) {
    const int d3 = d % 3;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int c = (d3 + b) % 3;
        prow[4 * d + b + 3 - 2 * c] = valid ? lut[c * 256 + ((v >> (8 * b)) & 255u)] : 0.f;
    }
}

// The K loop of one tile for one wave: acc (+ accs: H2's small products) = the wave's 32 pixels x 64 channels.  arow: this lane's pixel in the
// fp32 patch (rows of PROW floats) + 8 * half; wl: the weight planes in LDS.  Statement for statement the loop of conv1_x6.
template <bool H2, int PROW>
__device__ __forceinline__ void conv1_mma(const float* arow, const char* wl, int r, int half, c1_floatx16 (&acc)[2], c1_floatx16 (&accs)[2]) {
    constexpr int CH = H2 ? kH2ChunkBytes : kChunkBytes;
    constexpr int WROW = C1_CHUNKS * CH + 16;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc[0][i] = 0.f; acc[1][i] = 0.f; accs[0][i] = 0.f; accs[1][i] = 0.f; }
#pragma unroll
    for (int ky = 0; ky < 7; ++ky) {
#pragma unroll
        for (int jc = 0; jc < 2; ++jc) {
            const float* a = arow + ky * PROW + 16 * jc;
            const c1_f32x2 a0 = *reinterpret_cast<const c1_f32x2*>(a), a1 = *reinterpret_cast<const c1_f32x2*>(a + 2),
                           a2 = *reinterpret_cast<const c1_f32x2*>(a + 4), a3 = *reinterpret_cast<const c1_f32x2*>(a + 6);
            const int chunk = ky * 2 + jc;
            if constexpr (H2) {
                h2_u32x4 ah, al;
                split2_x8((h2_f32x4){a0.x, a0.y, a1.x, a1.y} * kC1PatchScale, (h2_f32x4){a2.x, a2.y, a3.x, a3.y} * kC1PatchScale, ah, al);
                const c1_f16x8 Ah = __builtin_bit_cast(c1_f16x8, ah), Al = __builtin_bit_cast(c1_f16x8, al);
                c1_f16x8 Bh[2], Bl[2];
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) {
                    const char* wp = wl + (cb * 32 + r) * WROW + chunk * CH + half * 16;
                    Bh[cb] = *reinterpret_cast<const c1_f16x8*>(wp);
                    Bl[cb] = *reinterpret_cast<const c1_f16x8*>(wp + 32);
                }
                accs[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Al, Bh[0], accs[0], 0, 0, 0);
                accs[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Al, Bh[1], accs[1], 0, 0, 0);
                accs[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Bl[0], accs[0], 0, 0, 0);
                accs[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Bl[1], accs[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Bh[0], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Bh[1], acc[1], 0, 0, 0);
                continue;
            }
            sp3_u32x4 ah, am, al;
            split3_x8((sp3_f32x4){a0.x, a0.y, a1.x, a1.y}, (sp3_f32x4){a2.x, a2.y, a3.x, a3.y}, ah, am, al);
            const c1_bf16x8 Ah = __builtin_bit_cast(c1_bf16x8, ah), Am = __builtin_bit_cast(c1_bf16x8, am),
                            Al = __builtin_bit_cast(c1_bf16x8, al);
            c1_bf16x8 Bh[2], Bm[2], Bl[2];
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
                const char* wp = wl + (cb * 32 + r) * WROW + chunk * CH + half * 16;
                Bh[cb] = *reinterpret_cast<const c1_bf16x8*>(wp);
                Bm[cb] = *reinterpret_cast<const c1_bf16x8*>(wp + 32);
                Bl[cb] = *reinterpret_cast<const c1_bf16x8*>(wp + 64);
            }
            // the six partial products, smallest first; the two accumulators alternate (no MFMA waits on the one before it)
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Al, Bh[0], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Al, Bh[1], acc[1], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Am, Bm[0], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Am, Bm[1], acc[1], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bl[0], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bl[1], acc[1], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Am, Bh[0], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Am, Bh[1], acc[1], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bm[0], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bm[1], acc[1], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bh[0], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bh[1], acc[1], 0, 0, 0);
        }
    }
}

// Hc, Wc: the canvas; OH = Hc / 2, OW = Wc / 2 multiples of 16.  n_tiles = N * (OH / 16) * (OW / 16), walked image by image, row of tiles by row
template <bool H2>
__global__ __launch_bounds__(512) void conv1_x6_canvas(const uint8_t* __restrict__ frags, const char* __restrict__ w_sp3, float* __restrict__ out,
                                                       float* __restrict__ gap, int n_tiles, const float* __restrict__ w_inv, int Hc, int Wc) {
#if __HIP_DEVICE_COMPILE__
    constexpr int CH = H2 ? kH2ChunkBytes : kChunkBytes;
    constexpr int UPR = C1_CHUNKS * CH / 16;
    constexpr int WROW = C1_CHUNKS * CH + 16;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* wl = smem;
    float* patch0 = reinterpret_cast<float*>(smem + C1_W_BYTES);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, half = lane >> 5;
    const int OH = Hc >> 1, OW = Wc >> 1;
    const int tiles_x = OW / C1C_T, tiles_img = (OH / C1C_T) * tiles_x;
    const int row_dw = Wc * 3 / 4;                             // dwords per image row (Wc a multiple of 4)

    for (int u = tid; u < 64 * UPR; u += 512) {
        const int n = u / UPR, q = u - n * UPR;
        *reinterpret_cast<sp3_u32x4*>(wl + n * WROW + q * 16) = *reinterpret_cast<const sp3_u32x4*>(w_sp3 + ((int64_t)n * UPR + q) * 16);
    }
    for (int i = tid; i < 2 * C1C_PATCH_FLOATS; i += 512) patch0[i] = 0.f;
    float* lut = patch0 + 2 * C1C_PATCH_FLOATS;
    for (int i = tid; i < 3 * 256; i += 512) {
        const int c = i >> 8;
        const float u = (float)(i & 255) / 255.0f;                                                      // as rn_preprocess
        lut[i] = c == 2 ? (u - 0.485f) / 0.229f : c == 1 ? (u - 0.456f) / 0.224f : (u - 0.406f) / 0.225f;
    }
    __syncthreads();

    unsigned raw[C1C_LOADS];
    // tile t: image, first output row / column, first input row, first dword of the window in an image row (negative left of the image)
    auto tile_geom = [&](int t, int& img, int& y0, int& x0, int& iy0, int& dw0) {
        img = t / tiles_img;
        const int rem = t - img * tiles_img;
        const int ty = rem / tiles_x;
        y0 = ty * C1C_T;
        x0 = (rem - ty * tiles_x) * C1C_T;
        iy0 = 2 * y0 - 3;
        dw0 = (6 * x0 - 12) / 4;
    };
    auto request = [&](int t) {
        int img, y0, x0, iy0, dw0;
        tile_geom(t, img, y0, x0, iy0, dw0);
        const unsigned* im = reinterpret_cast<const unsigned*>(frags + (int64_t)img * Hc * Wc * 3);
#pragma unroll
        for (int i = 0; i < C1C_LOADS; ++i) {
            const int e = tid + 512 * i;
            const int row = e / C1C_ROW_DW, d = e - row * C1C_ROW_DW;
            const int iy = iy0 + row, dw = dw0 + d;
            raw[i] = (row < C1C_PROWS && (unsigned)iy < (unsigned)Hc && (unsigned)dw < (unsigned)row_dw) ? im[iy * row_dw + dw] : 0u;
        }
    };
    auto deposit = [&](int t, float* patch) {
        int img, y0, x0, iy0, dw0;
        tile_geom(t, img, y0, x0, iy0, dw0);
#pragma unroll
        for (int i = 0; i < C1C_LOADS; ++i) {
            const int e = tid + 512 * i;
            const int row = e / C1C_ROW_DW, d = e - row * C1C_ROW_DW;
            if (row < C1C_PROWS)
                conv1_canvas_put4(patch + row * C1C_PROW, d, raw[i], (unsigned)(iy0 + row) < (unsigned)Hc && (unsigned)(dw0 + d) < (unsigned)row_dw, lut);
        }
    };

    int cur = 0;
    if ((int)blockIdx.x < n_tiles) {
        request(blockIdx.x);
        deposit(blockIdx.x, patch0);
    }
    __syncthreads();
    for (int t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        int img, y0, x0, iy0, dw0;
        tile_geom(t, img, y0, x0, iy0, dw0);
        const float* patch = patch0 + cur * C1C_PATCH_FLOATS;
        const int next = t + gridDim.x;
        if (next < n_tiles) request(next);                 // in flight under the MFMAs below

        // this lane's output pixel: rows 2 wave and 2 wave + 1 of the tile, 16 pixels each (A rows of the wave's 32x64 block)
        const int yl = 2 * wave + (r >> 4), xl = r & 15;
        const float* arow = patch + (2 * yl) * C1C_PROW + C1C_COL0 + 6 * xl + 8 * half;
        c1_floatx16 acc[2], accs[2];
        conv1_mma<H2, C1C_PROW>(arow, wl, r, half, acc, accs);
        // acc[cb][i]: channel cb*32 + r of the wave's pixel (i & 3) + 8 * (i >> 2) + 4 * half: row (i >> 3) of its two, column (i & 3) + 8 * ((i >> 2) & 1) + 4 * half
        if constexpr (H2) {   // the scales are powers of two: exact
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) acc[cb] = (acc[cb] + accs[cb]) * (w_inv[cb * 32 + r] * (1.f / kC1PatchScale));
        }
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int64_t pixg = ((int64_t)img * OH + y0 + 2 * wave + g) * OW + x0;   // first pixel of the row: a multiple of 16
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    out[(pixg + (i & 3) + 8 * (i >> 2) + 4 * half) * 64 + cb * 32 + r] = acc[cb][8 * g + i];
                if (gap) {   // the row's 16 pixels are one aligned group of the image's pixels, summed in conv1_x6's order
                    float s = 0.f;
#pragma unroll
                    for (int i = 0; i < 8; ++i) s += acc[cb][8 * g + i];
                    s += __shfl_xor(s, 32);
                    if (half == 0) gap[(pixg >> 4) * 64 + cb * 32 + r] = s;
                }
            }
        }
        if (next < n_tiles) deposit(next, patch0 + (cur ^ 1) * C1C_PATCH_FLOATS);   // the other buffer: nobody reads it during this tile
        __syncthreads();                                   // next patch complete, every wave done with this one
        cur ^= 1;
    }
#endif
}

// ---- the same stem on EVERY canvas (RELAX_RN_CANVAS_ANY: Hc, Wc any integers; host_logic.h, rn_stem_plan) ---------------------------------------
// What conv1_x6_canvas assumes and this form does not:
//   * the output map is OH = (Hc - 1) / 2 + 1 by OW = (Wc - 1) / 2 + 1 (torch's floor rule; Hc >> 1 on even sizes only) and need not be whole tiles:
//     ceil(OH / 16) x ceil(OW / 16) tiles per image, the K loop runs on the whole tile (pixels right of / below the map contract zeros or the
//     neighbouring rows' pixels: finite, never stored) and only the pixels inside the map are written;
//   * an image row is Wc * 3 bytes at ANY alignment (65 x 67: 13 065 bytes per image, the images of a batch start at every address mod 4).  A patch
//     row's window is still the 116 bytes from byte 6 x0 - 12 of the image row (a multiple of 3: byte k of it is channel k % 3); it is read as the 30
//     ALIGNED dwords that cover it from the address rounded down, and the deposit shifts by that address's two low bits.  A dword that would reach
//     outside the batch's bytes [0, N Hc Wc 3) - in front of the first image or behind the last row of the last one - is put together from the
//     bytes that lie inside instead: no read leaves the allocation.  Bytes of a dword that belong to the neighbouring row or image are
//     deposited as the zeros of the padding, by their position in the row;
//   * the fused 16-pixel group sums only where a group never crosses a row end (OW a multiple of 16; the launcher refuses `gap` otherwise and the
//     forward takes the mean from the raw output).
// The K loop, the split and the order of the products are conv1_mma's: a pixel has the bits conv1_x6_canvas gives it where both forms apply.
constexpr int C1A_WIN = 4 * C1C_ROW_DW;                    // 116 window bytes per patch row
constexpr int C1A_ROW_DW = C1C_ROW_DW + 1;                 // 30 aligned dwords cover them at every misalignment (116 + 3 bytes)
[[maybe_unused]] constexpr int C1A_LOADS = (C1C_PROWS * C1A_ROW_DW + 511) / 512;   // 3 dwords per thread and tile
static_assert(C1A_WIN - 1 + 3 < C1C_PROW, "every deposited byte lands inside its patch row");

template <bool H2>
__global__ __launch_bounds__(512) void conv1_x6_any(const uint8_t* __restrict__ frags, const char* __restrict__ w_sp3, float* __restrict__ out,
                                                    float* __restrict__ gap, int n_tiles, const float* __restrict__ w_inv, int Hc, int Wc, int64_t total_bytes) {
#if __HIP_DEVICE_COMPILE__
    constexpr int CH = H2 ? kH2ChunkBytes : kChunkBytes;
    constexpr int UPR = C1_CHUNKS * CH / 16;
    constexpr int WROW = C1_CHUNKS * CH + 16;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* wl = smem;
    float* patch0 = reinterpret_cast<float*>(smem + C1_W_BYTES);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, half = lane >> 5;
    const int OH = (Hc - 1) / 2 + 1, OW = (Wc - 1) / 2 + 1;
    const int tiles_x = (OW + C1C_T - 1) / C1C_T, tiles_img = ((OH + C1C_T - 1) / C1C_T) * tiles_x;
    const int row_bytes = Wc * 3;
    const uint64_t base_addr = reinterpret_cast<uint64_t>(frags);

    for (int u = tid; u < 64 * UPR; u += 512) {
        const int n = u / UPR, q = u - n * UPR;
        *reinterpret_cast<sp3_u32x4*>(wl + n * WROW + q * 16) = *reinterpret_cast<const sp3_u32x4*>(w_sp3 + ((int64_t)n * UPR + q) * 16);
    }
    for (int i = tid; i < 2 * C1C_PATCH_FLOATS; i += 512) patch0[i] = 0.f;
    float* lut = patch0 + 2 * C1C_PATCH_FLOATS;
    for (int i = tid; i < 3 * 256; i += 512) {
        const int c = i >> 8;
        const float u = (float)(i & 255) / 255.0f;                                                      // as rn_preprocess
        lut[i] = c == 2 ? (u - 0.485f) / 0.229f : c == 1 ? (u - 0.456f) / 0.224f : (u - 0.406f) / 0.225f;
    }
    __syncthreads();

    unsigned raw[C1A_LOADS];
    // tile t: image, first output row / column, first input row, first byte of the window in an image row (negative left of the image)
    auto tile_geom = [&](int t, int& img, int& y0, int& x0, int& iy0, int& win0) {
        img = t / tiles_img;
        const int rem = t - img * tiles_img;
        const int ty = rem / tiles_x;
        y0 = ty * C1C_T;
        x0 = (rem - ty * tiles_x) * C1C_T;
        iy0 = 2 * y0 - 3;
        win0 = 6 * x0 - 12;
    };
    // byte offset (in the batch) of the window of input row iy, and the two low bits of its address: the aligned dwords start that many bytes before it
    auto window = [&](int img, int iy, int win0, int64_t& g, int& a) {
        g = ((int64_t)img * Hc + iy) * row_bytes + win0;
        a = (int)((base_addr + (uint64_t)g) & 3u);
    };
    auto request = [&](int t) {
        int img, y0, x0, iy0, win0;
        tile_geom(t, img, y0, x0, iy0, win0);
#pragma unroll
        for (int i = 0; i < C1A_LOADS; ++i) {
            const int e = tid + 512 * i;
            const int row = e / C1A_ROW_DW, d = e - row * C1A_ROW_DW;
            const int iy = iy0 + row;
            unsigned v = 0u;
            if (row < C1C_PROWS && (unsigned)iy < (unsigned)Hc) {
                int64_t g;
                int a;
                window(img, iy, win0, g, a);
                const int64_t off = g - a + 4 * d;                  // (frags + off is dword-aligned)
                if (off >= 0 && off + 4 <= total_bytes) {
                    v = *reinterpret_cast<const unsigned*>(frags + off);
                } else {                                            // the ends of the batch: the bytes that exist
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (off + b >= 0 && off + b < total_bytes) v |= (unsigned)frags[off + b] << (8 * b);
                }
            }
            raw[i] = v;
        }
    };
    auto deposit = [&](int t, float* patch) {
        int img, y0, x0, iy0, win0;
        tile_geom(t, img, y0, x0, iy0, win0);
#pragma unroll
        for (int i = 0; i < C1A_LOADS; ++i) {
            const int e = tid + 512 * i;
            const int row = e / C1A_ROW_DW, d = e - row * C1A_ROW_DW;
            if (row >= C1C_PROWS) continue;
            const int iy = iy0 + row;
            const bool row_ok = (unsigned)iy < (unsigned)Hc;
            int64_t g;
            int a = 0;
            if (row_ok) window(img, iy, win0, g, a);               // (a row above / below the image: zeros at shift 0, every window byte once)
            float* prow = patch + row * C1C_PROW;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int k = 4 * d + b - a;                        // byte of the window
                if (k < 0 || k >= C1A_WIN) continue;
                const int c = k % 3;
                const int rb = win0 + k;                            // byte of the image row
                const bool ok = row_ok && rb >= 0 && rb < row_bytes;
                prow[k + 3 - 2 * c] = ok ? lut[c * 256 + ((raw[i] >> (8 * b)) & 255u)] : 0.f;   // (conv1_canvas_put4's column)
            }
        }
    };

    int cur = 0;
    if ((int)blockIdx.x < n_tiles) {
        request(blockIdx.x);
        deposit(blockIdx.x, patch0);
    }
    __syncthreads();
    for (int t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        int img, y0, x0, iy0, win0;
        tile_geom(t, img, y0, x0, iy0, win0);
        const float* patch = patch0 + cur * C1C_PATCH_FLOATS;
        const int next = t + gridDim.x;
        if (next < n_tiles) request(next);                 // in flight under the MFMAs below

        const int yl = 2 * wave + (r >> 4), xl = r & 15;
        const float* arow = patch + (2 * yl) * C1C_PROW + C1C_COL0 + 6 * xl + 8 * half;
        c1_floatx16 acc[2], accs[2];
        conv1_mma<H2, C1C_PROW>(arow, wl, r, half, acc, accs);
        if constexpr (H2) {   // the scales are powers of two: exact
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) acc[cb] = (acc[cb] + accs[cb]) * (w_inv[cb * 32 + r] * (1.f / kC1PatchScale));
        }
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int y = y0 + 2 * wave + g;
            if (y >= OH) continue;                             // (wave-uniform) a row below the map
            const int64_t pixg = ((int64_t)img * OH + y) * OW + x0;
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int col = (i & 3) + 8 * (i >> 2) + 4 * half;
                    if (x0 + col < OW) out[(pixg + col) * 64 + cb * 32 + r] = acc[cb][8 * g + i];
                }
                if (gap) {   // (OW a multiple of 16: the tile's row is whole, inside the map, and one aligned group of the image's pixels)
                    float s = 0.f;
#pragma unroll
                    for (int i = 0; i < 8; ++i) s += acc[cb][8 * g + i];
                    s += __shfl_xor(s, 32);
                    if (half == 0) gap[(pixg >> 4) * 64 + cb * 32 + r] = s;
                }
            }
        }
        if (next < n_tiles) deposit(next, patch0 + (cur ^ 1) * C1C_PATCH_FLOATS);   // the other buffer: nobody reads it during this tile
        __syncthreads();                                   // next patch complete, every wave done with this one
        cur ^= 1;
    }
#endif
}

int launch_conv1_x6_any(relax_handle* h, const uint8_t* frags, const void* w_sp3, float* out, float* gap_groups, int N, int Hc, int Wc, hipStream_t s,
                        const float* w_inv) {
    RELAX_REQUIRE(h, frags && w_sp3 && out && N > 0 && Hc > 0 && Wc > 0 && Hc <= 4096 && Wc <= 4096, "conv1_x6_any: bad arguments (canvas %d x %d)", Hc, Wc);
    const int OH = (Hc - 1) / 2 + 1, OW = (Wc - 1) / 2 + 1;
    RELAX_REQUIRE(h, !gap_groups || OW % 16 == 0, "conv1_x6_any: the fused spatial mean needs output rows of whole 16-pixel groups (%d x %d)", OH, OW);
    const int64_t tiles = (int64_t)N * ((OH + C1C_T - 1) / C1C_T) * ((OW + C1C_T - 1) / C1C_T);
    RELAX_REQUIRE(h, tiles < 0x7fffffff, "conv1_x6_any: %d images of %d x %d are too many tiles", N, Hc, Wc);
    static std::atomic<bool> lds_allowed_any[kMaxDevices];
    RELAX_TRY(allow_dynamic_lds(h, {reinterpret_cast<const void*>(&conv1_x6_any<false>), reinterpret_cast<const void*>(&conv1_x6_any<true>)}, C1C_LDS,
                                lds_allowed_any));
    const int n_tiles = (int)tiles;
    const int64_t total_bytes = (int64_t)N * Hc * Wc * 3;
    const double flops = 2.0 * N * (double)OH * OW * 64.0 * 147.0;
    const double bytes = (double)total_bytes + (double)N * OH * OW * 64 * 4;
    int span;
    RELAX_TRY(prof_begin(h, s, w_inv ? 5 : 2, flops, &span, bytes));
    const dim3 grid(n_tiles < 256 ? n_tiles : 256);
    if (w_inv)
        hipLaunchKernelGGL(conv1_x6_any<true>, grid, dim3(512), C1C_LDS, s, frags, static_cast<const char*>(w_sp3), out, gap_groups, n_tiles, w_inv, Hc, Wc,
                           total_bytes);
    else
        hipLaunchKernelGGL(conv1_x6_any<false>, grid, dim3(512), C1C_LDS, s, frags, static_cast<const char*>(w_sp3), out, gap_groups, n_tiles,
                           static_cast<const float*>(nullptr), Hc, Wc, total_bytes);
    if (hipGetLastError() != hipSuccess) { prof_abort(h, span); set_error(h, "conv1_x6_any: launch failed"); return RELAX_ERR_HIP; }
    RELAX_TRY(prof_end(h, s, span));
    return RELAX_OK;
}

// fp32 staging rows [64][224]: the packed conv1 rows in this kernel's K layout
static int conv1_staged(relax_handle* h, const float* w_packed, int kpad, ScopedDev& tmp, const char* what) {
    if (!tmp.alloc(h, 64 * C1_K, what)) return RELAX_ERR_NOMEM;
    hipLaunchKernelGGL(conv1_repack, dim3((64 * C1_K + 255) / 256), dim3(256), 0, nullptr, w_packed, kpad, tmp.p);
    return RELAX_OK;
}
// the conversion is through before the caller's scope frees the staging rows
static int conv1_converted(relax_handle* h, int rc) {
    if (hipDeviceSynchronize() != hipSuccess && rc == RELAX_OK) {
        set_error(h, "resnet50: conv1 weight conversion failed");
        rc = RELAX_ERR_HIP;
    }
    return rc;
}

// w_f32 [64][224] scratch -> w_sp3 [64][224 * 6 B]
int make_conv1_x6_weights(relax_handle* h, const float* w_packed, int kpad, void** w_sp3_out, DeviceOwner& mem) {
    const char* what = "the conv1 split-plane weights";
    ScopedDev tmp;
    RELAX_TRY(conv1_staged(h, w_packed, kpad, tmp, what));
    return conv1_converted(h, derive_sp3(h, mem, tmp.p, 64, C1_K, w_sp3_out, what));
}

// the same weights as two fp16 planes [64][224 * 4 B] with one power-of-two scale per filter (w_inv_out [64]: the inverse scales)
int make_conv1_h2_weights(relax_handle* h, const float* w_packed, int kpad, void** w_h2_out, float** w_inv_out, DeviceOwner& mem) {
    const char* what = "the conv1 fp16-plane weights";
    ScopedDev tmp;
    RELAX_TRY(conv1_staged(h, w_packed, kpad, tmp, what));
    return conv1_converted(h, derive_h2_rows(h, mem, tmp.p, 64, C1_K, w_h2_out, w_inv_out, what));
}

// frags uint8 [N,Hc,Wc,3] BGR -> out fp32 [N,Hc/2,Wc/2,64] (raw conv1), gap_groups [N*(Hc/2)(Wc/2)/16][64] (16-pixel sums) or null.
// w_inv != null: `w` holds fp16 planes (make_conv1_h2_weights) and the kernel runs its f16x2 form.  224 x 224 runs conv1_x6, compiled for that
// size; every other accepted canvas conv1_x6_canvas
int launch_conv1_x6(relax_handle* h, const uint8_t* frags, const void* w_sp3, float* out, float* gap_groups, int N, int Hc, int Wc, hipStream_t s,
                    const float* w_inv) {
    RELAX_REQUIRE(h, frags && w_sp3 && out && N > 0, "conv1_x6: bad arguments");
    const bool fixed = Hc == C1_HW && Wc == C1_HW;
    RELAX_REQUIRE(h, fixed || (Hc >= 2 * C1C_T && Wc >= 2 * C1C_T && Hc % (2 * C1C_T) == 0 && Wc % (2 * C1C_T) == 0),
                  "conv1_x6: canvas %d x %d: the output map must be whole 16 x 16 tiles", Hc, Wc);
    RELAX_REQUIRE(h, (int64_t)N * (Hc / 2) * (Wc / 2) / C1_TILE < 0x7fffffff, "conv1_x6: %d images of %d x %d are too many tiles", N, Hc, Wc);
    static std::atomic<bool> lds_allowed[kMaxDevices], lds_allowed_canvas[kMaxDevices];
    if (fixed)
        RELAX_TRY(allow_dynamic_lds(h, {reinterpret_cast<const void*>(&conv1_x6<false>), reinterpret_cast<const void*>(&conv1_x6<true>)}, C1_LDS, lds_allowed));
    else
        RELAX_TRY(allow_dynamic_lds(h, {reinterpret_cast<const void*>(&conv1_x6_canvas<false>), reinterpret_cast<const void*>(&conv1_x6_canvas<true>)}, C1C_LDS,
                                    lds_allowed_canvas));
    static_assert(C1_OPIX % C1_TILE == 0 && (C1_HW / 2) * (C1_HW / 2) == C1_OPIX, "the 224 kernel walks whole tiles");
    const int64_t opix = (int64_t)(Hc / 2) * (Wc / 2);
    const int n_tiles = (int)(N * (opix / C1_TILE));
    const double flops = 2.0 * N * (double)opix * 64.0 * 147.0;
    const double bytes = (double)N * ((double)Hc * Wc * 3 + (double)opix * 64 * 4);
    int span;
    RELAX_TRY(prof_begin(h, s, w_inv ? 5 : 2, flops, &span, bytes));
    const dim3 grid(n_tiles < 256 ? n_tiles : 256);
    if (fixed && w_inv)
        hipLaunchKernelGGL(conv1_x6<true>, grid, dim3(512), C1_LDS, s, frags, static_cast<const char*>(w_sp3), out, gap_groups, n_tiles, w_inv);
    else if (fixed)
        hipLaunchKernelGGL(conv1_x6<false>, grid, dim3(512), C1_LDS, s, frags, static_cast<const char*>(w_sp3), out, gap_groups, n_tiles,
                           static_cast<const float*>(nullptr));
    else if (w_inv)
        hipLaunchKernelGGL(conv1_x6_canvas<true>, grid, dim3(512), C1C_LDS, s, frags, static_cast<const char*>(w_sp3), out, gap_groups, n_tiles, w_inv,
                           Hc, Wc);
    else
        hipLaunchKernelGGL(conv1_x6_canvas<false>, grid, dim3(512), C1C_LDS, s, frags, static_cast<const char*>(w_sp3), out, gap_groups, n_tiles,
                           static_cast<const float*>(nullptr), Hc, Wc);
    if (hipGetLastError() != hipSuccess) { prof_abort(h, span); set_error(h, "conv1_x6: launch failed"); return RELAX_ERR_HIP; }
    RELAX_TRY(prof_end(h, s, span));
    return RELAX_OK;
}

}  // namespace relax
