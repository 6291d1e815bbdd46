// ViT attention visualisation on gfx950: the CLS row of the last block's attention and its overlay on full frames.
//
// Reference semantics (file:line in xinyiW915/ReLaX-VQA):
//   src/extractor/visualise_vit.py:241-250   get_last_selfattention: blocks 0..10, then block 11's softmax(q k^T / 8)
//   src/extractor/visualise_vit.py:123-127   Block.forward(return_attention=True)
//   src/extractor/visualise_vit.py:353-369   visualize_attention: attn[0, :, 0, 1:] (the CLS query against the 196 patches)
//   src/demo_visual.py:12-25                 map_attention_to_original(.., patch_size): per-patch values painted at their source
//                                            positions, / max * 255 -> uint8, applyColorMap(JET), addWeighted(frame, .6, heat, .4, 0);
//                                            patch_size 8 / 16 / 32 and any slot count up to (448 / 8)^2 (relax_attention_overlay_ex)
#include "relax_internal.h"

namespace relax {

constexpr int AM_KPT = 4;               // keys per thread: thread j owns keys j, j + 256, ... (up to 1024 tokens; 197 tokens: one key each)
constexpr int AM_KPT_WIDE = 17;         // ... of the second instantiation: up to 4352 tokens (host::kVitMaxPatches + 1 = 4097 needs 17)
constexpr int AM_HD = 64;              // head_dim of vit_tiny / vit_small / vit_base: the scale 64^-0.5 is exactly 1/8
constexpr int OV_MAX_SLOTS = (448 / 8) * (448 / 8);   // 3136: the largest canvas of the fragment stage at its smallest patch
constexpr int OV_SPT = (OV_MAX_SLOTS + 255) / 256;    // slots per thread of overlay_levels: thread j owns slots j, j + 256, ...

// ---- 1. CLS-row attention ---------------------------------------------------------------------------------------------------
// value j of a qkv row: fp32 rows [3*dim], or two fp16 planes (csrc/h2.h: chunks of [16 hi][16 lo], value = (hi + lo) / s_qkv;
// hi + lo is exact in fp32 and 1 / s_qkv is a power of two, so the value is the one the forward's attention reads)
template <bool H2>
__device__ inline void load16(const void* qkv, int64_t row, int ld_vals, int col, float inv_s, float* v) {
    if (H2) {
        const char* c = static_cast<const char*>(qkv) + row * (int64_t)ld_vals * 4 + (int64_t)(col >> 4) * 64;   // col % 16 == 0
        const uint4 u[4] = {reinterpret_cast<const uint4*>(c)[0], reinterpret_cast<const uint4*>(c)[1],
                            reinterpret_cast<const uint4*>(c)[2], reinterpret_cast<const uint4*>(c)[3]};
        const _Float16* hi = reinterpret_cast<const _Float16*>(&u[0]);
        const _Float16* lo = reinterpret_cast<const _Float16*>(&u[2]);
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = ((float)hi[j] + (float)lo[j]) * inv_s;
    } else {
        const float4* p = reinterpret_cast<const float4*>(static_cast<const float*>(qkv) + row * (int64_t)ld_vals + col);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float4 f = p[j];
            v[4 * j] = f.x; v[4 * j + 1] = f.y; v[4 * j + 2] = f.z; v[4 * j + 3] = f.w;
        }
    }
}

__device__ inline float block_reduce_256(float x, float* red, bool is_max) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float y = __shfl_xor(x, o);
        x = is_max ? fmaxf(x, y) : x + y;
    }
    const int w = threadIdx.x >> 6;
    __syncthreads();                       // (red may still be read by the previous reduction)
    if ((threadIdx.x & 63) == 0) red[w] = x;
    __syncthreads();
    return is_max ? fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) : (red[0] + red[1]) + (red[2] + red[3]);
}

// one workgroup per (image, head); thread j owns keys j, j + 256, ... (at most KPT; 197 tokens: key j alone, the arithmetic of the
// one-key-per-thread form bit for bit).  fp32 logits (q_0 . k_j sequential FMA, * 1/8), max subtracted, fp32 sum in a fixed tree: an
// image's row depends on nothing else in the batch.
template <bool H2, int KPT>
__global__ __launch_bounds__(256) void vit_cls_attention(const void* __restrict__ qkv, float inv_s, float* __restrict__ out, int heads, int ntok) {
    __shared__ float q[AM_HD];
    __shared__ float red[4];
    const int n = blockIdx.x / heads, hd = blockIdx.x % heads;
    const int dim = heads * AM_HD, ld = 3 * dim;
    const int j = threadIdx.x;
    if (j < AM_HD / 16) load16<H2>(qkv, (int64_t)n * ntok, ld, hd * AM_HD + j * 16, inv_s, q + j * 16);
    __syncthreads();
    float logit[KPT];
    float lmax = -INFINITY;
#pragma unroll
    for (int t = 0; t < KPT; ++t) {
        const int key = j + 256 * t;
        logit[t] = -INFINITY;
        if (key < ntok) {
            const int64_t row = (int64_t)n * ntok + key;
            float acc = 0.f;
#pragma unroll
            for (int c = 0; c < AM_HD; c += 16) {
                float k[16];
                load16<H2>(qkv, row, ld, dim + hd * AM_HD + c, inv_s, k);
#pragma unroll
                for (int d = 0; d < 16; ++d) acc = fmaf(q[c + d], k[d], acc);
            }
            logit[t] = acc * 0.125f;
        }
        lmax = fmaxf(lmax, logit[t]);
    }
    const float mx = block_reduce_256(lmax, red, true);
    float e[KPT];
    float lsum = 0.f;
#pragma unroll
    for (int t = 0; t < KPT; ++t) {
        e[t] = j + 256 * t < ntok ? expf(logit[t] - mx) : 0.f;
        lsum = t == 0 ? e[0] : lsum + e[t];
    }
    const float sum = block_reduce_256(lsum, red, false);
#pragma unroll
    for (int t = 0; t < KPT; ++t)
        if (j + 256 * t < ntok) out[(int64_t)blockIdx.x * ntok + j + 256 * t] = e[t] / sum;
}

int launch_vit_cls_attention(relax_handle* h, const void* qkv, bool planes, float s_qkv, float* out, int N, int ntok, int heads, hipStream_t s) {
    RELAX_REQUIRE(h, qkv && out && N > 0 && heads > 0, "vit_cls_attention: bad arguments");
    RELAX_REQUIRE(h, ntok > 0 && ntok <= 256 * AM_KPT_WIDE, "vit_cls_attention: ntok=%d (1 .. %d)", ntok, 256 * AM_KPT_WIDE);
    const dim3 grid((unsigned)(N * heads));
    const bool wide = ntok > 256 * AM_KPT;   // (197 and 785 tokens keep the instantiation they always ran)
    if (planes) {
        RELAX_REQUIRE(h, s_qkv > 0.f && s_qkv < 3.0e38f, "vit_cls_attention: bad qkv scale");
        // (fp16 planes come from the f16x2 forward: attention_h2 at 197 tokens, attention_stream_h2 at any other count)
        if (wide) hipLaunchKernelGGL((vit_cls_attention<true, AM_KPT_WIDE>), grid, dim3(256), 0, s, qkv, 1.f / s_qkv, out, heads, ntok);
        else hipLaunchKernelGGL((vit_cls_attention<true, AM_KPT>), grid, dim3(256), 0, s, qkv, 1.f / s_qkv, out, heads, ntok);
    } else {
        if (wide) hipLaunchKernelGGL((vit_cls_attention<false, AM_KPT_WIDE>), grid, dim3(256), 0, s, qkv, 1.f, out, heads, ntok);
        else hipLaunchKernelGGL((vit_cls_attention<false, AM_KPT>), grid, dim3(256), 0, s, qkv, 1.f, out, heads, ntok);
    }
    RELAX_HIP_CHECK(h, hipGetLastError());
    return RELAX_OK;
}

// ---- 3. overlay ---------------------------------------------------------------------------------------------------------------
// Levels: one workgroup per frame writes level[t][py][px] (uint8, [ph][pw]) for the whole patch grid.  A slot k < counts[t] whose
// position lies inside the grid paints its patch; when two slots name the same patch the later one wins (the reference's loop
// overwrites).  Out-of-range positions paint nothing (relax_gather_patches gives them a zero tile).  max is over the whole frame,
// so it includes 0 unless the painted patches cover every pixel; level = trunc((double)v / (double)max * 255) as numpy computes it
// on the reference's float64 array.  max <= 0 (undefined in the reference): every level is 0; so are negative and NaN values.
__global__ __launch_bounds__(256) void overlay_levels(const int32_t* __restrict__ positions, const int32_t* __restrict__ counts,
                                                      const float* __restrict__ vals, int slots, int ph, int pw, int edge,
                                                      uint8_t* __restrict__ lvl) {
    extern __shared__ int key[];   // [slots]: the flat patch a slot paints, -1 for none
    __shared__ float red[4];
    const int t = blockIdx.x;
    const int npatch = ph * pw;
    uint8_t* L = lvl + (int64_t)t * npatch;
    const int cnt = counts[t];
    for (int k = threadIdx.x; k < slots; k += 256) {
        int my = -1;
        if (k < cnt) {
            const int y = positions[((int64_t)t * slots + k) * 2], x = positions[((int64_t)t * slots + k) * 2 + 1];
            if ((unsigned)y < (unsigned)ph && (unsigned)x < (unsigned)pw) my = y * pw + x;
        }
        key[k] = my;
    }
    for (int i = threadIdx.x; i < npatch; i += 256) L[i] = 0;
    __syncthreads();
    // a slot is final when no later slot names its patch
    uint32_t final_mask = 0;
    float lmax = -INFINITY, lpainted = 0.f;
#pragma unroll 1
    for (int j = 0; j < OV_SPT; ++j) {
        const int k = threadIdx.x + 256 * j;
        if (k >= slots) break;
        const int my = key[k];
        bool final_ = my >= 0;
        for (int k2 = k + 1; k2 < slots && final_; ++k2) final_ = key[k2] != my;
        if (final_) {
            final_mask |= 1u << j;
            lmax = fmaxf(lmax, vals[(int64_t)t * slots + k]);
            lpainted += 1.f;
        }
    }
    float mx = block_reduce_256(lmax, red, true);
    const float painted = block_reduce_256(lpainted, red, false);
    if (edge || painted < (float)npatch) mx = fmaxf(mx, 0.f);
#pragma unroll 1
    for (int j = 0; j < OV_SPT; ++j) {
        if (!((final_mask >> j) & 1u)) continue;
        const int k = threadIdx.x + 256 * j;
        int l = 0;
        if (mx > 0.f) {
            const double q = (double)vals[(int64_t)t * slots + k] / (double)mx * 255.0;
            l = q > 0.0 ? (int)q : 0;
            l = l > 255 ? 255 : l;
        }
        L[key[k]] = (uint8_t)l;
    }
}

// out = (6 frame + 4 lut[level] + 5) / 10 per byte: rint(0.6 a + 0.4 b) of cv2.addWeighted for every (a, b) byte pair
__device__ inline uint32_t blend_u8x4(uint32_t a, uint32_t b4p5_0, uint32_t b4p5_1, uint32_t b4p5_2, uint32_t b4p5_3) {
    return (((a & 255u) * 6u + b4p5_0) / 10u) | (((((a >> 8) & 255u) * 6u + b4p5_1) / 10u) << 8) |
           (((((a >> 16) & 255u) * 6u + b4p5_2) / 10u) << 16) | ((((a >> 24) * 6u + b4p5_3) / 10u) << 24);
}

// W % 16 == 0, 16-byte aligned frames and rows: one thread per 16 pixels of a row (48 bytes = 3 x 16-byte loads and stores).
// psh = log2(patch size).  At 16 (and inside one patch at 32) that is one patch column: one level and one colour per thread; at 8 the
// 16 pixels are two patches - bytes 0..23 take the level of patch 2g (colours c*), bytes 24..47 that of patch 2g+1 (colours d*).
__global__ __launch_bounds__(256) void overlay_blend16(const uint8_t* __restrict__ frames, int64_t frame_stride, int H, int W,
                                                       int psh, int ph, int pw, const uint8_t* __restrict__ lvl,
                                                       const uint8_t* __restrict__ lut, uint8_t* __restrict__ out) {
    const int t = blockIdx.y;
    const int gw = W / 16;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H * gw) return;
    const int y = i / gw, g = i - y * gw;
    const int py = y >> psh;
    const int pxa = (g * 16) >> psh, pxb = (g * 16 + 8) >> psh;
    const int l = (py < ph && pxa < pw) ? lvl[((int64_t)t * ph + py) * pw + pxa] : 0;
    const int lb = (py < ph && pxb < pw) ? lvl[((int64_t)t * ph + py) * pw + pxb] : 0;
    const uint32_t c0 = 4u * lut[3 * l] + 5u, c1 = 4u * lut[3 * l + 1] + 5u, c2 = 4u * lut[3 * l + 2] + 5u;
    const uint32_t d0 = 4u * lut[3 * lb] + 5u, d1 = 4u * lut[3 * lb + 1] + 5u, d2 = 4u * lut[3 * lb + 2] + 5u;
    const int64_t off = ((int64_t)y * W + (int64_t)g * 16) * 3;
    const uint4* src = reinterpret_cast<const uint4*>(frames + t * frame_stride + off);
    uint4* dst = reinterpret_cast<uint4*>(out + (int64_t)t * H * W * 3 + off);
    const uint4 a = src[0], b = src[1], c = src[2];
    // byte 16 u + 4 w + j of the 48 has channel (16 u + 4 w + j) % 3
    dst[0] = make_uint4(blend_u8x4(a.x, c0, c1, c2, c0), blend_u8x4(a.y, c1, c2, c0, c1), blend_u8x4(a.z, c2, c0, c1, c2),
                        blend_u8x4(a.w, c0, c1, c2, c0));
    dst[1] = make_uint4(blend_u8x4(b.x, c1, c2, c0, c1), blend_u8x4(b.y, c2, c0, c1, c2), blend_u8x4(b.z, d0, d1, d2, d0),
                        blend_u8x4(b.w, d1, d2, d0, d1));
    dst[2] = make_uint4(blend_u8x4(c.x, d2, d0, d1, d2), blend_u8x4(c.y, d0, d1, d2, d0), blend_u8x4(c.z, d1, d2, d0, d1),
                        blend_u8x4(c.w, d2, d0, d1, d2));
}

// any shape / alignment: one thread per pixel
__global__ __launch_bounds__(256) void overlay_blend1(const uint8_t* __restrict__ frames, int64_t frame_stride, int H, int W,
                                                      int psh, int ph, int pw, const uint8_t* __restrict__ lvl,
                                                      const uint8_t* __restrict__ lut, uint8_t* __restrict__ out) {
    const int t = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)H * W) return;
    const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
    const int py = y >> psh, px = x >> psh;
    const int l = (py < ph && px < pw) ? lvl[((int64_t)t * ph + py) * pw + px] : 0;
    const uint8_t* a = frames + t * frame_stride + i * 3;
    uint8_t* o = out + ((int64_t)t * H * W + i) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (uint8_t)((6u * a[c] + 4u * lut[3 * l + c] + 5u) / 10u);
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace relax

using namespace relax;

extern "C" {

int relax_attention_overlay_ex(relax_handle* h, const uint8_t* frames, int64_t frame_stride, int T, int H, int W, int patch_size,
                               int slots, const int32_t* positions, const int32_t* counts, const float* patch_values,
                               const uint8_t* lut_bgr, uint8_t* out, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, frames && positions && counts && patch_values && lut_bgr && out, "relax_attention_overlay: NULL pointer");
    RELAX_REQUIRE(h, T > 0 && H > 0 && W > 0, "relax_attention_overlay: bad shape T=%d H=%d W=%d", T, H, W);
    RELAX_REQUIRE(h, patch_size == 8 || patch_size == 16 || patch_size == 32, "relax_attention_overlay: patch_size=%d is not built (8, 16 or 32)",
                  patch_size);
    RELAX_REQUIRE(h, slots > 0 && slots <= OV_MAX_SLOTS, "relax_attention_overlay: slots=%d must be in [1,%d]", slots, OV_MAX_SLOTS);
    RELAX_REQUIRE(h, frame_stride >= (int64_t)H * W * 3 || T == 1, "relax_attention_overlay: frame stride smaller than a frame");
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int psh = patch_size == 8 ? 3 : patch_size == 16 ? 4 : 5;
    const int ph = H >> psh, pw = W >> psh;
    const size_t map_bytes = (size_t)T * ph * pw;
    RELAX_TRY(ensure_buf(h, h->scratch, map_bytes > 0 ? map_bytes : 16));
    uint8_t* lvl = static_cast<uint8_t*>(h->scratch.p);
    const int edge = (H % patch_size) != 0 || (W % patch_size) != 0;
    hipLaunchKernelGGL(overlay_levels, dim3(T), dim3(256), sizeof(int) * (size_t)slots, s, positions, counts, patch_values, slots, ph, pw,
                       edge, lvl);
    const bool vec = W % 16 == 0 && (frame_stride % 16 == 0 || T == 1) && aligned16(frames) && aligned16(out);
    if (vec) {
        const int64_t items = (int64_t)H * (W / 16);
        hipLaunchKernelGGL(overlay_blend16, dim3((unsigned)((items + 255) / 256), T), dim3(256), 0, s, frames, frame_stride, H, W, psh, ph,
                           pw, lvl, lut_bgr, out);
    } else {
        const int64_t items = (int64_t)H * W;
        hipLaunchKernelGGL(overlay_blend1, dim3((unsigned)((items + 255) / 256), T), dim3(256), 0, s, frames, frame_stride, H, W, psh, ph,
                           pw, lvl, lut_bgr, out);
    }
    RELAX_HIP_CHECK(h, hipGetLastError());
    return RELAX_OK;
}

int relax_attention_overlay(relax_handle* h, const uint8_t* frames, int64_t frame_stride, int T, int H, int W,
                            const int32_t* positions, const int32_t* counts, const float* patch_values,
                            const uint8_t* lut_bgr, uint8_t* out, relax_stream stream) {
    return relax_attention_overlay_ex(h, frames, frame_stride, T, H, W, RELAX_PATCH, RELAX_TOP_N, positions, counts, patch_values, lut_bgr,
                                      out, stream);
}

}  // extern "C"
