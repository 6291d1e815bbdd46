// Streaming attention under "f16x2" for any token count, 64-d heads:  softmax(q k^T / 8) v  on the two fp16 planes the qkv GEMM's epilogue
// writes (csrc/h2.h: x * s = hi + lo, chunks of [16 hi][16 lo], one static scale for the whole qkv tensor), with an online softmax over key
// tiles of 64.  It is attention_h2.hip's arithmetic in attention_stream.hip's structure:
//   * both contractions as three partial products (lo hi, hi lo, hi hi - smallest first) on v_mfma_f32_32x32x16_f16, fp32 accumulation;
//   * alpha = log2(e) / 8 / s^2 applied in one fma in front of v_exp_f32; probabilities (<= 1) split as planes of e * 2^14 (NOT folded into
//     the exponent: attention_h2.hip's header records why); V's scale, the 2^14 and the output scale folded into 1 / l;
//   * one workgroup = one (image, head, block of 128 queries): 4 waves x 32 queries, a lane owns ONE query with its lane ^ 32 partner.  It
//     walks the ceil(ntok / 64) key tiles in order and owns all of them - no split over keys, no atomics: the same bits on every run and
//     for every batch an image is sent in;
//   * update: padding keys (key >= ntok) are set to -inf BEFORE the tile maximum; m' = max(m, tile max); a = exp2(fl(-m' alpha) - fl(-m alpha)), 0 on
//     the first tile (-inf - -inf is never formed); l = l a + sum p; o = o a + (the tile's V^T P^T, summed on its own).  Their bound is
//     ntok * 2^14 * 2^15 < 2^42 at 4097 keys.
// Staging: the K and V rows of a tile are 256 contiguous bytes of planes per key and go global -> LDS by LDS-DMA straight into the fragment
// images of attention_h2.hip (the sixteen 16-byte units of a row XOR-permuted by f(key & 15) on the SOURCE offset; K read with ds_read_b128,
// V with the transposing ds_read_b64_tr_b16), so that kernel's address maps - and their known bank behaviour - hold per tile.  Two tile
// buffers: tile t + 1 is requested before the math of tile t and awaited (s_waitcnt vmcnt(0)) in front of the ONE barrier that ends tile t;
// a buffer is read only after the barrier that follows its wait, and overwritten only after the barrier that follows its last read.  One
// tile's DMA in flight, never more.  Every operand goes through a buffer resource over the image's own ntok rows: rows past ntok arrive as
// zeros; padding QUERY rows are clamped on load and dropped on store by the output resource's range (no branch around the stores).
// LDS: 2 buffers x (K image + V image) x 64 keys x 256 B = 64 KB, two workgroups per CU (128 of 160 KB).  Registers: 256 VGPRs a lane, no
// AGPRs, no scratch (__launch_bounds__(256, 2): the compiler fills the budget of two waves per SIMD, which is what two workgroups of four
// waves per CU are; the kernel's live set is 172 + the tile's 32 accumulators): occupancy 2 waves per SIMD, 8 per CU.
#include "relax_internal.h"
#include "host_logic.h"
#include "h2.h"

namespace relax {

typedef float sh_floatx16 __attribute__((ext_vector_type(16)));
typedef float sh_f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 sh_f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned sh_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned sh_u32x2 __attribute__((ext_vector_type(2)));
typedef short sh_i16x4 __attribute__((__vector_size__(4 * sizeof(short))));

constexpr int SH_QB = host::kAttStreamH2QBlock;
constexpr int SH_KT = host::kAttStreamH2KeyTile;
constexpr int SH_THREADS = SH_QB * 2;            // 4 waves: 32 queries each, two lanes per query
constexpr int SH_WAVES = SH_THREADS / 64;
constexpr int SH_ROW = host::kAttStreamH2RowBytes;
constexpr int SH_IMG = SH_KT * SH_ROW;           // one image (K or V) of one tile: 16384
constexpr int SH_BUF = 2 * SH_IMG;               // K image, V image
constexpr int SH_LDS = 2 * SH_BUF;               // two tiles resident
constexpr int SH_PPW = SH_IMG / 1024 / SH_WAVES; // DMA pieces (4 rows = 1024 B) per wave and image: 4
static_assert(SH_THREADS == 256 && SH_KT == 64 && SH_ROW == 256, "the task maps below are written for 256 threads, 64-key tiles and 256-byte rows");
static_assert(SH_LDS == host::kAttStreamH2Lds, "the plan's LDS size is this kernel's");
static_assert(SH_PPW * SH_WAVES * 1024 == SH_IMG, "the pieces divide over the waves");

__device__ inline int sh_f(int k) {   // the unit permutation of row k (k & 15 matters): attention_h2.hip's
    return ((k >> 2) & 1) | ((k & 1) << 1) | (((k >> 3) & 1) << 2) | (((k >> 1) & 1) << 3);
}
__device__ inline sh_f16x8 sh_frag(const sh_u32x4 v) { return __builtin_bit_cast(sh_f16x8, v); }

// dev_scalars (operator-level entry only): {alpha, out_mul} computed on the device from the tensor's measured maximum
__global__ __launch_bounds__(SH_THREADS, 2) void attention_stream_h2(const char* __restrict__ qkvp, char* __restrict__ out_h2, int ntok, int heads,
                                                                     int qblocks, int key_tiles, float alpha, float out_mul,
                                                                     const float* __restrict__ dev_scalars) {
#if __HIP_DEVICE_COMPILE__   // the host pass only needs the launch stub (no __amdgpu_buffer_rsrc_t there)
    if (dev_scalars) {
        alpha = dev_scalars[0];
        out_mul = dev_scalars[1];
    }
    extern __shared__ __attribute__((aligned(256))) char smem[];
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int li = lane & 31, half = lane >> 5;
    const int dim = heads * 64;
    const int ldb = 3 * dim * 4;              // bytes of a token's qkv row of planes
    const int item = blockIdx.x;
    const int qb = item % qblocks;
    const int head = (item / qblocks) % heads;
    const int64_t img = item / qblocks / heads;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    // (ntok + one tile) * ldb < 2^31: host::att_stream_h2_plan
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(qkvp + img * ntok * ldb), 0, ntok * ldb, 0x00020000);

    // K and V rows of key tile kt_ -> buffer buf_: 4 rows per DMA instruction, lane l fills position l & 15 of row 4 piece + (l >> 4) with the
    // source unit (l & 15) ^ f(row); rows at or past ntok lie beyond the resource and arrive as zeros
    const int kv_col = (dim + head * 64) * 4;
    auto dma_tile = [&](int kt_, int buf_) {
#pragma unroll
        for (int which = 0; which < 2; ++which)
#pragma unroll
            for (int j = 0; j < SH_PPW; ++j) {
                const int piece = wave_u * SH_PPW + j;
                const int row_ = piece * 4 + (lane >> 4);
                const int src_ = (lane & 15) ^ sh_f(row_);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(smem + buf_ * SH_BUF + which * SH_IMG + piece * 1024),
                                                         16, (kt_ * SH_KT + row_) * ldb + kv_col + which * (dim * 4) + src_ * 16, 0, 0, 0);
            }
    };
#define SH_WAIT_DMA() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")

    dma_tile(0, 0);
    // the planes of this lane's query: d = 16 s + 8 half .. + 7 for s = 0 .. 3, hi and lo (a clamped row for the padding queries)
    const int q = qb * SH_QB + wave * 32 + li;
    sh_u32x4 qh[4], ql[4];
    {
        const int q_ofs = (q < ntok ? q : ntok - 1) * ldb + head * 256 + half * 16;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            qh[s] = __builtin_bit_cast(sh_u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, q_ofs + s * 64, 0, 0));
            ql[s] = __builtin_bit_cast(sh_u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, q_ofs + s * 64 + 32, 0, 0));
        }
    }

    // K fragment addresses: key 32 t + li of the tile, d step s, plane p: position ((4 s + 2 p + half) ^ f(li)) of the row
    const int fk = sh_f(li);
    int kaddr[4][2];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int p = 0; p < 2; ++p) kaddr[s][p] = li * SH_ROW + ((((2 * p + half) ^ fk) << 4) ^ (s << 6));
    // V^T fragment addresses (transposed reads): lane = 16 g + 4 q + p; half = g >> 1, chunk = 2 dt + (g & 1); block row q = key
    // 16 c + 4 half + q (+ 8 for the second read of a fragment), columns 4 p .. 4 p + 3 of the chunk's 16 d of one plane
    int vaddr[2][2][2];   // [read j][dt][plane], key step c adds 4096 c
    {
        const int g = lane >> 4, qq = (lane >> 2) & 3, p = lane & 3;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int ko = 4 * (g >> 1) + qq + 8 * j;
            const int fv = sh_f(ko);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int pl = 0; pl < 2; ++pl) {
                    const int u = 4 * (2 * dt + (g & 1)) + 2 * pl + (p >> 1);
                    vaddr[j][dt][pl] = SH_IMG + ko * SH_ROW + ((u ^ fv) << 4) + 8 * (p & 1);
                }
        }
    }

    float m = -INFINITY, m_shift = 0.f, l = 0.f;   // m: the running maximum of the RAW sums (alpha > 0); m_shift = fl(-m alpha)
    sh_floatx16 oacc[2];            // oacc[dt][r] = O(query, d = dt*32 + (r&3) + 8*(r>>2) + 4*half) * (s 2^14), unnormalised
#pragma unroll
    for (int r = 0; r < 16; ++r) { oacc[0][r] = 0.f; oacc[1][r] = 0.f; }

    SH_WAIT_DMA();
    __syncthreads();          // tile 0 has landed (every wave waited for its own pieces before the barrier)

    for (int kt = 0; kt < key_tiles; ++kt) {
        const int cur = (kt & 1) * SH_BUF;
        // the other buffer was last read during tile kt - 1, and the barrier that ended it lies behind every wave
        if (kt + 1 < key_tiles) dma_tile(kt + 1, (kt + 1) & 1);

        // ---- scores: sacc[t][r] * alpha = score(this query, key kt*64 + 32 t + (r&3) + 8*(r>>2) + 4*half) * log2(e) ---------------------
        sh_floatx16 sacc[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[t][r] = 0.f;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const sh_f16x8 k_hi = *reinterpret_cast<const sh_f16x8*>(smem + cur + t * (32 * SH_ROW) + kaddr[s][0]);
                const sh_f16x8 k_lo = *reinterpret_cast<const sh_f16x8*>(smem + cur + t * (32 * SH_ROW) + kaddr[s][1]);
                sacc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(k_lo, sh_frag(qh[s]), sacc[t], 0, 0, 0);
                sacc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(k_hi, sh_frag(ql[s]), sacc[t], 0, 0, 0);
                sacc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(k_hi, sh_frag(qh[s]), sacc[t], 0, 0, 0);
            }
        }

        // ---- online softmax ------------------------------------------------------------------------------------------------------------
        if (kt == key_tiles - 1) {    // (workgroup-uniform) only the last tile holds padding keys: masked before the tile max
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (kt * SH_KT + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * half >= ntok) sacc[t][r] = -INFINITY;
        }
        float tmax = -INFINITY;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, sacc[t][r]);
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));     // (finite: every tile holds at least one real key)
        const float m_new = fmaxf(m, tmax);
        const float shift = -m_new * alpha;
        // what was accumulated so far carries exp2(. + m_shift) with the ROUNDED m_shift: the rescale is the difference of the two rounded
        // shifts (exp2(m alpha + shift) would be off by m_shift's rounding, 4e-6 at logits of 60, once per move of the maximum)
        const float a = m == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(shift - m_shift);   // first tile: nothing accumulated yet
        m_shift = shift;
        float psum = 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float e = __builtin_amdgcn_exp2f(fmaf(sacc[t][r], alpha, shift));
                sacc[t][r] = e;
                psum += e;
            }
        psum += __shfl_xor(psum, 32);
        l = l * a + psum;
        m = m_new;

        // ---- output: O^T[d, query] += V^T P^T over 4 steps of 16 keys; probabilities (<= 1) as planes of e * 2^14.  Registers 8*(c&1) .. +7
        // of score tile c>>1 are keys 16c + 8*(j>>2) + 4*half + (j&3): the B fragment of step c; the A fragment = the same 8 keys of d = dt*32 + li
        // The tile's products are summed in accumulators of their own and join the running ones in ONE fma per value (o = o a + tile): the
        // running sums are rounded once per tile, not at each of the tile's 12 MFMAs - at 4097 keys the latter measured 8.6 times torch-CPU
        // fp32's distance from fp64 on near-uniform rows, this form 1/4 of that
        sh_floatx16 tacc[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) { tacc[0][r] = 0.f; tacc[1][r] = 0.f; }
#pragma unroll
        for (int c = 0; c < SH_KT / 16; ++c) {
            sh_u32x4 p_hi, p_lo;
            split2_x8((h2_f32x4){sacc[c >> 1][8 * (c & 1) + 0], sacc[c >> 1][8 * (c & 1) + 1], sacc[c >> 1][8 * (c & 1) + 2],
                                 sacc[c >> 1][8 * (c & 1) + 3]} * 16384.f,
                      (h2_f32x4){sacc[c >> 1][8 * (c & 1) + 4], sacc[c >> 1][8 * (c & 1) + 5], sacc[c >> 1][8 * (c & 1) + 6],
                                 sacc[c >> 1][8 * (c & 1) + 7]} * 16384.f,
                      p_hi, p_lo);
#define SH_TR(addr_) __builtin_bit_cast(sh_u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16(                            \
                         (__attribute__((address_space(3))) sh_i16x4*)(smem + cur + (addr_) + c * (16 * SH_ROW))))
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                sh_u32x4 vf[2];   // [plane]
#pragma unroll
                for (int pl = 0; pl < 2; ++pl) {
                    const sh_u32x2 a_ = SH_TR(vaddr[0][dt][pl]), b_ = SH_TR(vaddr[1][dt][pl]);
                    vf[pl] = (sh_u32x4){a_.x, a_.y, b_.x, b_.y};
                }
                tacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(sh_frag(vf[1]), sh_frag(p_hi), tacc[dt], 0, 0, 0);
                tacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(sh_frag(vf[0]), sh_frag(p_lo), tacc[dt], 0, 0, 0);
                tacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(sh_frag(vf[0]), sh_frag(p_hi), tacc[dt], 0, 0, 0);
            }
#undef SH_TR
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            oacc[0][r] = fmaf(oacc[0][r], a, tacc[0][r]);
            oacc[1][r] = fmaf(oacc[1][r], a, tacc[1][r]);
        }
        SH_WAIT_DMA();            // this wave's pieces of tile kt + 1 have landed ...
        __syncthreads();          // ... so have everyone's, and every wave is done with this tile's buffer
    }

    // ---- epilogue (attention_h2's): the lane ^ 32 partner holds the 4-value runs of d in between; after swapping two runs per tile each lane
    // owns two units of 8 consecutive d.  The planes leave through a buffer resource that covers the item's image exactly: the padding
    // queries (rows >= ntok) are out of its range and their stores are dropped
    const float inv = out_mul / l;
    const __amdgpu_buffer_rsrc_t rs_out =
        __builtin_amdgcn_make_buffer_rsrc(out_h2 + img * ntok * ((int64_t)dim * 4), 0, ntok * dim * 4, 0x00020000);
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
        float own[16], got[8];
#pragma unroll
        for (int r = 0; r < 16; ++r) own[r] = oacc[dt][r] * inv;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) got[4 * u + j] = __shfl_xor(half ? own[8 * u + j] : own[8 * u + 4 + j], 32);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            sh_f32x4 lo4, hi4;
            if (half == 0) {
                lo4 = (sh_f32x4){own[8 * u], own[8 * u + 1], own[8 * u + 2], own[8 * u + 3]};
                hi4 = (sh_f32x4){got[4 * u], got[4 * u + 1], got[4 * u + 2], got[4 * u + 3]};
            } else {
                lo4 = (sh_f32x4){got[4 * u], got[4 * u + 1], got[4 * u + 2], got[4 * u + 3]};
                hi4 = (sh_f32x4){own[8 * u + 4], own[8 * u + 5], own[8 * u + 6], own[8 * u + 7]};
            }
            const int d0 = head * 64 + dt * 32 + 16 * u + 8 * half;
            h2_u32x4 ph, pl;
            split2_x8(lo4, hi4, ph, pl);                                           // (the output scale is folded into inv)
            const int vo = q * (dim * 4) + (int)h2_offset(d0);                     // (q < ntok + 128: below 2^31 with the plan's bound)
            __builtin_amdgcn_raw_buffer_store_b128(ph, rs_out, vo, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b128(pl, rs_out, vo + 32, 0, 0);
        }
    }
#undef SH_WAIT_DMA
#endif
}

static int stream_h2_plan(relax_handle* h, int Nimg, int heads, int ntok, host::AttStreamH2Plan* p) {
    std::string err;
    if (!host::att_stream_h2_plan(Nimg, heads, ntok, p, err)) {
        set_error(h, "%s", err.c_str());
        return RELAX_ERR_INVALID;
    }
    static std::atomic<bool> lds_allowed[kMaxDevices];
    RELAX_TRY(allow_dynamic_lds(h, {reinterpret_cast<const void*>(&attention_stream_h2)}, SH_LDS, lds_allowed));
    return RELAX_OK;
}

// qkv_planes: fp16 planes [Nimg * ntok][3 * dim * 4 B] of qkv * s_qkv; out_planes: [Nimg * ntok][dim * 4 B] of the attention output * out_scale
// (the layout attention_h2 writes)
int launch_attention_stream_h2(relax_handle* h, const void* qkv_planes, float s_qkv, void* out_planes, float out_scale, int Nimg, int ntok, int heads,
                               hipStream_t s) {
    RELAX_REQUIRE(h, qkv_planes && out_planes, "attention_stream_h2: NULL operand");
    RELAX_REQUIRE(h, s_qkv > 0.f && s_qkv < 3.0e38f && out_scale > 0.f && out_scale < 3.0e38f, "attention_stream_h2: bad scales");
    host::AttStreamH2Plan p;
    RELAX_TRY(stream_h2_plan(h, Nimg, heads, ntok, &p));
    // log2(e) / 8 and the two operand scales folded into the logits; the probabilities' 2^14, V's scale and the output scale into 1 / l
    const float alpha = (float)(0.125 * 1.44269504088896341 / ((double)s_qkv * (double)s_qkv));
    const float out_mul = (float)((double)out_scale / ((double)s_qkv * 16384.0));
    hipLaunchKernelGGL(attention_stream_h2, dim3((unsigned)p.items), dim3(SH_THREADS), SH_LDS, s, static_cast<const char*>(qkv_planes),
                       static_cast<char*>(out_planes), ntok, heads, p.qblocks, p.key_tiles, alpha, out_mul, static_cast<const float*>(nullptr));
    RELAX_HIP_CHECK(h, hipGetLastError());
    return RELAX_OK;
}

// operator-level entry (relax_op_attention_ex under "f16x2" with "att_h2" and "att_h2_stream"): fp32 qkv in, fp32 out.  The planes are made
// here with ONE scale for the whole tensor from its measured maximum, everything on the device (attention_h2_op_steps)
int launch_attention_stream_h2_op(relax_handle* h, const float* qkv, float* out, int Nimg, int ntok, int heads, hipStream_t s) {
    RELAX_REQUIRE(h, qkv && out, "attention_stream_h2 (operator): NULL operand");
    host::AttStreamH2Plan p;
    RELAX_TRY(stream_h2_plan(h, Nimg, heads, ntok, &p));
    const int dim = heads * 64;
    const int64_t rows = (int64_t)Nimg * ntok;
    RELAX_REQUIRE(h, rows <= (int64_t)INT32_MAX, "attention_stream_h2 (operator): %d images of %d tokens pass 2^31 - 1 rows", Nimg, ntok);
    return attention_h2_op_steps(h, qkv, out, rows, dim, s, [&](const char* Qp, char* Op, const float* tab) -> int {
        hipLaunchKernelGGL(attention_stream_h2, dim3((unsigned)p.items), dim3(SH_THREADS), SH_LDS, s, Qp, Op, ntok, heads, p.qblocks, p.key_tiles, 0.f, 0.f, tab);
        RELAX_HIP_CHECK(h, hipGetLastError());
        return RELAX_OK;
    });
}

}  // namespace relax
