// Streaming attention for any token count, 64-d heads:  softmax(q k^T / 8) v  with an online softmax over key tiles of 32
// (src/extractor/visualise_vit_layer.py:93-106).  The single-tile kernels (attention_197x64, attention_x6, attention_h2) hold every
// key of an (image, head) on the chip at once, which ends at 224 keys; a DINO ViT at patch 8 has 785 tokens.
//
// One workgroup = one (image, head, block of 128 queries): 4 waves x 32 queries, a lane owns ONE query (with its lane ^ 32 partner).
// It walks the ceil(ntok / 32) key tiles in order and owns all of them - no split over keys, no atomics: the same bits on every run.
//   scores   S^T[key, query] = K Q^T : the key on the MFMA row (register) axis, the query on the lane - as in the single-tile kernels, so
//            a lane's 16 accumulators are 16 keys of its own query: tile max / exp2 / sum are register-local plus one lane ^ 32 exchange.
//   update   m' = max(m, tile max); alpha = exp2(m - m') (0 on the first tile: m = -inf is never subtracted from -inf); l = l alpha + sum p;
//            the output accumulators are scaled by alpha.  Padding keys (key >= ntok) are set to -inf BEFORE the tile max.
//   output   O^T[d, query] += V^T P^T : the probabilities stay where the scores were (the B operand of the next MFMA), and the output's
//            query axis is the lane too, so alpha and 1 / l apply without any transposition.
// Two arithmetics:
//   F32  v_mfma_f32_32x32x2_f32 on fp32 rows (the arithmetic of attention_197x64): K [32][68], V [32][72] floats in LDS
//   X6   bf16x6: v_mfma_f32_32x32x16_bf16 on the three bf16 planes of every operand, six partial products, smallest first (the arithmetic
//        and the plane images of attention_x6.hip; the V^T image keeps its permuted key order)
// Every operand load goes through a buffer resource over the image's own ntok rows: a row at or past ntok arrives as zeros (padding
// keys of the last tile), padding QUERY rows are clamped to the last real row on load and never stored.  The next tile's K / V rows are
// requested into registers before the current tile's MFMAs and written to LDS (split into planes under X6) after them.
#include "relax_internal.h"
#include "host_logic.h"
#include "sp3.h"
#include "h2.h"

namespace relax {

typedef float as_f32x16 __attribute__((ext_vector_type(16)));
typedef float as_f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 as_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned as_u32x4 __attribute__((ext_vector_type(4)));

constexpr int AS_THREADS = host::kAttStreamQBlock * 2;   // 4 waves: 32 queries each, two lanes per query
constexpr int AS_KT = host::kAttStreamKeyTile;
[[maybe_unused]] constexpr int AS_KLD = host::kAttStreamKLdF32, AS_VLD = host::kAttStreamVLdF32;
constexpr int AS_KROW = host::kAttStreamKRowX6, AS_VROW = host::kAttStreamVRowX6;
static_assert(AS_THREADS == 256 && AS_KT == 32, "the task maps below are written for 256 threads and 32-key tiles");
static_assert(AS_KROW == 4 * kChunkBytes + 16 && AS_VROW == 2 * kChunkBytes + 16, "plane images: chunks of csrc/sp3.h + one 16-byte pad");

__device__ inline as_bf16x8 as_frag(const as_u32x4 v) { return __builtin_bit_cast(as_bf16x8, v); }

template <int ARITH, int OUT_PLANES, bool OUT_F32>   // ARITH: host::kAttStreamF32 / kAttStreamX6; outputs as attention_x6
__global__ __launch_bounds__(AS_THREADS) void attention_stream(const float* __restrict__ qkv, float* __restrict__ out, char* __restrict__ out_planes,
                                                               int ntok, int heads, int qblocks, int key_tiles, float out_scale) {
#if __HIP_DEVICE_COMPILE__   // the host pass only needs the launch stub (no __amdgpu_buffer_rsrc_t there)
    constexpr bool X6 = ARITH == host::kAttStreamX6;
    constexpr int K_BYTES = X6 ? AS_KT * AS_KROW : AS_KT * AS_KLD * 4;
    constexpr int V_BYTES = X6 ? 64 * AS_VROW : AS_KT * AS_VLD * 4;
    static_assert(K_BYTES + V_BYTES == (X6 ? host::kAttStreamLdsX6 : host::kAttStreamLdsF32), "the plan's LDS size is this kernel's");
    __shared__ __attribute__((aligned(16))) char smem[K_BYTES + V_BYTES];
    char* const Kimg = smem;
    char* const Vimg = smem + K_BYTES;
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int li = lane & 31, half = lane >> 5;
    const int dim = heads * 64, ld = 3 * dim;
    const int item = blockIdx.x;
    const int qb = item % qblocks;
    const int head = (item / qblocks) % heads;
    const int64_t img = item / qblocks / heads;
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(qkv + img * ntok * ld), 0, ntok * ld * 4, 0x00020000);   // (< 2^31: host::att_stream_plan)
    const float kQScale = 0.125f * 1.44269504088896341f;   // head_dim^-0.5 and log2(e) folded into Q: the exponential is one v_exp_f32

    // ---- this lane's query -------------------------------------------------------------------------------------------------------
    const int q = qb * host::kAttStreamQBlock + wave * 32 + li;
    const int q_ofs = ((q < ntok ? q : ntok - 1) * ld + head * 64) * 4;
    [[maybe_unused]] as_f32x4 qf[8];       // F32: d = 8 j + 4 half .. + 3
    [[maybe_unused]] as_u32x4 qp[4][3];    // X6: [16-deep d step][plane], d = 16 s + 8 half .. + 7
    if (X6) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const as_f32x4 a = __builtin_bit_cast(as_f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, q_ofs + (16 * s + 8 * half) * 4, 0, 0));
            const as_f32x4 b = __builtin_bit_cast(as_f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, q_ofs + (16 * s + 8 * half + 4) * 4, 0, 0));
            sp3_u32x4 hi, mid, lo;
            split3_x8(a * kQScale, b * kQScale, hi, mid, lo);
            qp[s][0] = hi; qp[s][1] = mid; qp[s][2] = lo;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            qf[j] = __builtin_bit_cast(as_f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, q_ofs + (8 * j + 4 * half) * 4, 0, 0)) * kQScale;
    }

    // ---- key tile staging: thread -> (key tid >> 3, 8 d of K) and (d = lane, keys 8 wave .. + 7 of V) ------------------------------------
    as_f32x4 kraw[2];
    float vraw[8];
    const int k_ofs = ((tid >> 3) * ld + dim + head * 64 + (tid & 7) * 8) * 4;
    const int v_ofs = (wave * 8 * ld + 2 * dim + head * 64 + lane) * 4;
    auto request_tile = [&](int kt) {
        const int t_ofs = kt * AS_KT * ld * 4;
        kraw[0] = __builtin_bit_cast(as_f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, t_ofs + k_ofs, 0, 0));
        kraw[1] = __builtin_bit_cast(as_f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, t_ofs + k_ofs + 16, 0, 0));
#pragma unroll
        for (int j = 0; j < 8; ++j) vraw[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, t_ofs + v_ofs + j * ld * 4, 0, 0));
    };
    auto store_tile = [&]() {
        const int key = tid >> 3, d8 = tid & 7;
        if (X6) {
            sp3_u32x4 hi, mid, lo;
            split3_x8(kraw[0], kraw[1], hi, mid, lo);
            char* d = Kimg + key * AS_KROW + (d8 >> 1) * kChunkBytes + (d8 & 1) * 16;
            *reinterpret_cast<sp3_u32x4*>(d) = hi;
            *reinterpret_cast<sp3_u32x4*>(d + 32) = mid;
            *reinterpret_cast<sp3_u32x4*>(d + 64) = lo;
            // V^T image [d][2 chunks of 16 keys][3 planes][16]: key offset ko inside its chunk sits at position 8 h + 4 (g4 >> 1) + (ko & 3) with
            // g4 = ko >> 2, h = g4 & 1 - the order in which the score accumulators hold the keys, so P feeds the next MFMA unshuffled
            sp3_u32x2 h0, m0, l0, h1, m1, l1;
            split3_x4((sp3_f32x4){vraw[0], vraw[1], vraw[2], vraw[3]}, h0, m0, l0);
            split3_x4((sp3_f32x4){vraw[4], vraw[5], vraw[6], vraw[7]}, h1, m1, l1);
            char* v = Vimg + lane * AS_VROW + (wave >> 1) * kChunkBytes + (wave & 1) * 8;
            *reinterpret_cast<sp3_u32x2*>(v) = h0;
            *reinterpret_cast<sp3_u32x2*>(v + 16) = h1;
            *reinterpret_cast<sp3_u32x2*>(v + 32) = m0;
            *reinterpret_cast<sp3_u32x2*>(v + 48) = m1;
            *reinterpret_cast<sp3_u32x2*>(v + 64) = l0;
            *reinterpret_cast<sp3_u32x2*>(v + 80) = l1;
        } else {
            float* kd = reinterpret_cast<float*>(Kimg) + key * AS_KLD + d8 * 8;
            *reinterpret_cast<as_f32x4*>(kd) = kraw[0];
            *reinterpret_cast<as_f32x4*>(kd + 4) = kraw[1];
            float* vd = reinterpret_cast<float*>(Vimg) + wave * 8 * AS_VLD + lane;
#pragma unroll
            for (int j = 0; j < 8; ++j) vd[j * AS_VLD] = vraw[j];
        }
    };

    float m = -INFINITY, l = 0.f;
    as_f32x16 oacc[2];   // oacc[dt][r] = O(query, d = dt*32 + (r&3) + 8*(r>>2) + 4*half), unnormalised
#pragma unroll
    for (int r = 0; r < 16; ++r) { oacc[0][r] = 0.f; oacc[1][r] = 0.f; }

    request_tile(0);
    for (int kt = 0; kt < key_tiles; ++kt) {
        if (kt > 0) __syncthreads();          // every wave is done with the previous tile's images
        store_tile();
        __syncthreads();
        if (kt + 1 < key_tiles) request_tile(kt + 1);   // in flight during this tile's MFMAs

        // ---- scores: sacc[r] = score(this query, key kt*32 + (r&3) + 8*(r>>2) + 4*half) * log2(e) -----------------------------------------
        as_f32x16 sacc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
        if (X6) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const char* kp = Kimg + li * AS_KROW + s * kChunkBytes + half * 16;
                const as_bf16x8 k0 = *reinterpret_cast<const as_bf16x8*>(kp);
                const as_bf16x8 k1 = *reinterpret_cast<const as_bf16x8*>(kp + 32);
                const as_bf16x8 k2 = *reinterpret_cast<const as_bf16x8*>(kp + 64);
                sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k2, as_frag(qp[s][0]), sacc, 0, 0, 0);
                sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k1, as_frag(qp[s][1]), sacc, 0, 0, 0);
                sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k0, as_frag(qp[s][2]), sacc, 0, 0, 0);
                sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k1, as_frag(qp[s][0]), sacc, 0, 0, 0);
                sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k0, as_frag(qp[s][1]), sacc, 0, 0, 0);
                sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k0, as_frag(qp[s][0]), sacc, 0, 0, 0);
            }
        } else {
            const float* kp = reinterpret_cast<const float*>(Kimg) + li * AS_KLD + 4 * half;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const as_f32x4 kf = *reinterpret_cast<const as_f32x4*>(kp + 8 * j);
                sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, qf[j].x, sacc, 0, 0, 0);
                sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, qf[j].y, sacc, 0, 0, 0);
                sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, qf[j].z, sacc, 0, 0, 0);
                sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, qf[j].w, sacc, 0, 0, 0);
            }
        }

        // ---- online softmax ------------------------------------------------------------------------------------------------------------
        float tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = kt * AS_KT + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (key >= ntok) sacc[r] = -INFINITY;     // padding keys: masked before the tile max
            tmax = fmaxf(tmax, sacc[r]);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));     // (finite: every tile holds at least one real key)
        const float m_new = fmaxf(m, tmax);
        const float alpha = m == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m - m_new);   // first tile: nothing accumulated yet, no exp(-inf - -inf)
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float e = __builtin_amdgcn_exp2f(sacc[r] - m_new);
            sacc[r] = e;
            psum += e;
        }
        psum += __shfl_xor(psum, 32);
        l = l * alpha + psum;
        m = m_new;
#pragma unroll
        for (int r = 0; r < 16; ++r) { oacc[0][r] *= alpha; oacc[1][r] *= alpha; }

        // ---- output: O^T[d, query] += V^T P^T ------------------------------------------------------------------------------------------
        if (X6) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {     // registers 8c .. 8c+7 are keys 16c + 8*(j>>2) + 4*half + (j&3): the B fragment of step c
                sp3_u32x4 p0, p1, p2;
                split3_x8((sp3_f32x4){sacc[8 * c], sacc[8 * c + 1], sacc[8 * c + 2], sacc[8 * c + 3]},
                          (sp3_f32x4){sacc[8 * c + 4], sacc[8 * c + 5], sacc[8 * c + 6], sacc[8 * c + 7]}, p0, p1, p2);
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    const char* vp = Vimg + (dt * 32 + li) * AS_VROW + c * kChunkBytes + half * 16;
                    const as_bf16x8 v0 = *reinterpret_cast<const as_bf16x8*>(vp);
                    const as_bf16x8 v1 = *reinterpret_cast<const as_bf16x8*>(vp + 32);
                    const as_bf16x8 v2 = *reinterpret_cast<const as_bf16x8*>(vp + 64);
                    oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v2, as_frag(p0), oacc[dt], 0, 0, 0);
                    oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v1, as_frag(p1), oacc[dt], 0, 0, 0);
                    oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v0, as_frag(p2), oacc[dt], 0, 0, 0);
                    oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v1, as_frag(p0), oacc[dt], 0, 0, 0);
                    oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v0, as_frag(p1), oacc[dt], 0, 0, 0);
                    oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v0, as_frag(p0), oacc[dt], 0, 0, 0);
                }
            }
        } else {
            const float* vb = reinterpret_cast<const float*>(Vimg) + li;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = (r & 3) + 8 * (r >> 2) + 4 * half;
                const float v0 = vb[key * AS_VLD], v1 = vb[key * AS_VLD + 32];
                oacc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(v0, sacc[r], oacc[0], 0, 0, 0);
                oacc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(v1, sacc[r], oacc[1], 0, 0, 0);
            }
        }
    }

    // ---- epilogue (attention_x6's): the lane ^ 32 partner holds the 4-value runs of d in between; after swapping two runs per tile each
    // lane owns two units of 8 consecutive d:  half 0: d = dt*32 + 0..7 and 16..23,  half 1: d = dt*32 + 8..15 and 24..31
    const float inv = 1.0f / l;
    const int64_t orow = img * ntok + q;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
        float own[16], got[8];
#pragma unroll
        for (int r = 0; r < 16; ++r) own[r] = oacc[dt][r] * inv;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) got[4 * u + j] = __shfl_xor(half ? own[8 * u + j] : own[8 * u + 4 + j], 32);
        if (q < ntok) {     // padding queries are never stored
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                as_f32x4 lo4, hi4;
                if (half == 0) {
                    lo4 = (as_f32x4){own[8 * u], own[8 * u + 1], own[8 * u + 2], own[8 * u + 3]};
                    hi4 = (as_f32x4){got[4 * u], got[4 * u + 1], got[4 * u + 2], got[4 * u + 3]};
                } else {
                    lo4 = (as_f32x4){got[4 * u], got[4 * u + 1], got[4 * u + 2], got[4 * u + 3]};
                    hi4 = (as_f32x4){own[8 * u + 4], own[8 * u + 5], own[8 * u + 6], own[8 * u + 7]};
                }
                const int d0 = head * 64 + dt * 32 + 16 * u + 8 * half;
                if (OUT_PLANES == 1) store_sp3_x8(out_planes + orow * ((int64_t)dim * 6), d0, lo4, hi4);
                if (OUT_PLANES == 2) store_h2_x8(out_planes + orow * ((int64_t)dim * 4), d0, lo4, hi4, out_scale);
                if (OUT_F32) {
                    *reinterpret_cast<as_f32x4*>(out + orow * dim + d0) = lo4;
                    *reinterpret_cast<as_f32x4*>(out + orow * dim + d0 + 4) = hi4;
                }
            }
        }
    }
#endif
}

static int stream_plan(relax_handle* h, int Nimg, int heads, int ntok, int arith, host::AttStreamPlan* p) {
    std::string err;
    if (!host::att_stream_plan(Nimg, heads, ntok, arith, p, err)) {
        set_error(h, "%s", err.c_str());
        return RELAX_ERR_INVALID;
    }
    return RELAX_OK;
}

int launch_attention_stream_f32(relax_handle* h, const float* qkv, float* out, int Nimg, int ntok, int heads, hipStream_t s) {
    RELAX_REQUIRE(h, qkv && out, "attention_stream_f32: NULL operand");
    host::AttStreamPlan p;
    RELAX_TRY(stream_plan(h, Nimg, heads, ntok, host::kAttStreamF32, &p));
    hipLaunchKernelGGL((attention_stream<host::kAttStreamF32, 0, true>), dim3((unsigned)p.items), dim3(AS_THREADS), 0, s, qkv, out,
                       static_cast<char*>(nullptr), ntok, heads, p.qblocks, p.key_tiles, 1.f);
    RELAX_HIP_CHECK(h, hipGetLastError());
    return RELAX_OK;
}

int launch_attention_stream_x6(relax_handle* h, const float* qkv, float* out, void* out_planes, int Nimg, int ntok, int heads, hipStream_t s,
                               float out_h2_scale) {
    RELAX_REQUIRE(h, qkv && (out || out_planes), "attention_stream_x6: NULL operand");
    RELAX_REQUIRE(h, !(out_h2_scale > 0.f) || (out_planes && !out), "attention_stream_x6: the fp16-plane output goes alone");
    host::AttStreamPlan p;
    RELAX_TRY(stream_plan(h, Nimg, heads, ntok, host::kAttStreamX6, &p));
    const dim3 grid((unsigned)p.items), block(AS_THREADS);
    char* op = static_cast<char*>(out_planes);
    constexpr int X6 = host::kAttStreamX6;
    if (out_h2_scale > 0.f)
        hipLaunchKernelGGL((attention_stream<X6, 2, false>), grid, block, 0, s, qkv, out, op, ntok, heads, p.qblocks, p.key_tiles, out_h2_scale);
    else if (out && op)
        hipLaunchKernelGGL((attention_stream<X6, 1, true>), grid, block, 0, s, qkv, out, op, ntok, heads, p.qblocks, p.key_tiles, 1.f);
    else if (op)
        hipLaunchKernelGGL((attention_stream<X6, 1, false>), grid, block, 0, s, qkv, out, op, ntok, heads, p.qblocks, p.key_tiles, 1.f);
    else
        hipLaunchKernelGGL((attention_stream<X6, 0, true>), grid, block, 0, s, qkv, out, op, ntok, heads, p.qblocks, p.key_tiles, 1.f);
    RELAX_HIP_CHECK(h, hipGetLastError());
    return RELAX_OK;
}

}  // namespace relax

using namespace relax;

extern "C" int relax_op_attention_ex(relax_handle* h, const float* qkv, float* out, int Nimg, int ntok, int heads, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, qkv && out, "relax_op_attention_ex: NULL operand");
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the arithmetic the ViT forward's attention runs under this "gemm_precision": f16x2 planes under 3 with "att_h2" and "att_h2_stream",
    // bf16x6 under 2 and otherwise under 3, exact fp32 under 0 and 1
    if (h->gemm.precision == 3 && h->gemm.att_h2 && h->gemm.att_h2_stream) return launch_attention_stream_h2_op(h, qkv, out, Nimg, ntok, heads, s);
    if (h->gemm.precision >= 2) return launch_attention_stream_x6(h, qkv, out, nullptr, Nimg, ntok, heads, s, 0.f);
    return launch_attention_stream_f32(h, qkv, out, Nimg, ntok, heads, s);
}
