// ViT layer-stack taps (get_intermediate_layers, src/extractor/visualise_vit_layer.py:252-260: the final norm of the output of each of
// the last n blocks): the normed CLS row and mean | max | population std over the normed patch tokens of ONE tap in ONE launch, read off
// the fp32 residual stream X.  The normed tokens never exist in HBM.
//
// A workgroup of 16 waves owns one image's channels [slice * dim / S, (slice + 1) * dim / S) and makes three passes over the image's rows:
//   1. row statistics: one wave per row as layernorm_rows (csrc/layers.hip) has it - lane l holds float4s l, l + 64, l + 128 - mean and rstd
//      into LDS (two floats per row, ntok <= 4097: 32 KB; with the group partials 59 KB of the 64 KB a workgroup may declare).  This is the
//      HBM read of X.  The next row of a wave is loaded before the current one is reduced.  Slice 0's wave 0 writes the normed CLS row.
//   2. per (channel, token group): sum and max of the normed values, recomputed from X, mean[row], rstd[row], g, b.
//   3. per (channel, token group): the squared deviations from the channel mean, recomputed the same way.
// S = 1 where the images alone fill the card; with fewer images S = 2 .. 4 workgroups share an image, each repeating pass 1 (a row's
// statistics need the whole row) and keeping 1 / S of the channels in passes 2 and 3.  The S workgroups of an image are given ids that are
// congruent modulo 8, so they run on ONE XCD and share its L2: the first of them to touch a row brings it from HBM, the others' pass 1 is
// expected to hit L2.  Passes 2 and 3 re-read the image's rows (ntok * dim * 4 bytes: 605 KB for ViT-B at 197 tokens): expected to hit L2
// where the images in flight on an XCD fit its 4 MB, the Infinity Cache otherwise (256 images of ViT-B are 155 MB of its 256 MB); neither
// is a read of HBM.  What they cost instead of an HBM round trip of the normed tensor is the re-evaluation of (v - mean) * rstd * g + b,
// three VALU operations per value and pass.
//
// The bits are those of layernorm_rows<0> followed by vit_token_stats (csrc/vit.hip): the same expressions in the same order - the row sums
// (x + y) + (z + w) then the xor butterfly, rstd = 1 / sqrtf(var + eps), four token groups of stride 4 combined as (g0 + g1) + (g2 + g3),
// the mean pass before the squared-deviation pass.  Where those two kernels' ISA has a fused multiply-add (the variance's dx * dx + dy * dy,
// the last step of the normed value, the squared-deviation accumulation) this one writes fmaf, and nowhere else does a product meet a sum
// here, so the compiler's contraction has nothing left to decide.  A channel's chain of sums is the same whichever slice owns it.
#include "relax_internal.h"

namespace relax {

constexpr int kTapWaves = 16;
constexpr int kTapThreads = kTapWaves * 64;
constexpr int kTapMaxTok = 4097;   // host::kVitMaxPatches + 1
constexpr int kTapMaxDim = 768;    // launch_layernorm's limit: three float4s per lane
constexpr int kTapMaxSlices = 4;   // pass 1 is repeated per slice: beyond 4 it costs more than the idle CUs it fills
constexpr int kTapTargetGroups = 512;   // two workgroups per CU (their LDS and waves fit twice)

__device__ inline float tap_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// X [N, ntok, dim] -> cls_out [N, dim] (the normed row 0; may be NULL), pooled_out [N, 3 dim] (mean | max | std over the normed rows
// 1 .. ntok - 1; may be NULL).  dim % (64 S) == 0, dim <= 768, 2 <= ntok <= 4097.  grid = 8 S ceil(N / 8), block = 1024: workgroup id ->
// image (id % 8) + 8 (id / (8 S)), slice (id / 8) % S.
__global__ __launch_bounds__(kTapThreads) void vit_norm_token_stats(const float* __restrict__ X, const float* __restrict__ g,
                                                                    const float* __restrict__ b, float eps, float* __restrict__ cls_out,
                                                                    float* __restrict__ pooled_out, int N, int dim, int ntok, int S) {
    __shared__ float2 s_row[kTapMaxTok];       // (mean, rstd) of each row
    __shared__ float s_sum[4][kTapMaxDim];     // per token group: the sums, later the squared deviations
    __shared__ float s_max[4][kTapMaxDim];
    __shared__ float s_mean[kTapMaxDim];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int id = blockIdx.x;
    const int slice = (id >> 3) % S;
    const int64_t n = (id & 7) + 8 * (id / (8 * S));
    if (n >= N) return;   // uniform over the workgroup
    const float* xb = X + n * ntok * dim;
    const int nvec = dim >> 2;

    // ---- pass 1: layernorm_rows' statistics, one wave per row; without a pooled output only the CLS row is needed
    const int nrows = pooled_out ? ntok : 1;
    float4 nx[3];
    if (wave < nrows) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int i = lane + 64 * j;
            nx[j] = i < nvec ? reinterpret_cast<const float4*>(xb + (int64_t)wave * dim)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    for (int row = wave; row < nrows; row += kTapWaves) {   // wave-uniform
        float4 v[3];
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 3; ++j) v[j] = nx[j];
        if (row + kTapWaves < nrows) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int i = lane + 64 * j;
                nx[j] = i < nvec ? reinterpret_cast<const float4*>(xb + (int64_t)(row + kTapWaves) * dim)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
        const float mean = tap_wave_sum(s) / (float)dim;
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int i = lane + 64 * j;
            if (i < nvec) {
                const float dx = v[j].x - mean, dy = v[j].y - mean, dz = v[j].z - mean, dw = v[j].w - mean;
                q += fmaf(dx, dx, dy * dy) + fmaf(dz, dz, dw * dw);
            }
        }
        const float rstd = 1.0f / sqrtf(tap_wave_sum(q) / (float)dim + eps);
        if (lane == 0) s_row[row] = make_float2(mean, rstd);
        if (row == 0 && cls_out && slice == 0) {
            const float4* g4 = reinterpret_cast<const float4*>(g);
            const float4* b4 = reinterpret_cast<const float4*>(b);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int i = lane + 64 * j;
                if (i < nvec) {
                    const float4 gg = g4[i], bb = b4[i];
                    float4 o;
                    o.x = fmaf((v[j].x - mean) * rstd, gg.x, bb.x);
                    o.y = fmaf((v[j].y - mean) * rstd, gg.y, bb.y);
                    o.z = fmaf((v[j].z - mean) * rstd, gg.z, bb.z);
                    o.w = fmaf((v[j].w - mean) * rstd, gg.w, bb.w);
                    reinterpret_cast<float4*>(cls_out + n * dim)[i] = o;
                }
            }
        }
    }
    if (!pooled_out) return;   // uniform over the grid
    __syncthreads();

    // ---- passes 2 and 3: vit_token_stats over the patch rows 1 .. npatch.  Item (grp, lc) = token group grp of the slice's channel lc, lc
    // fastest, so a wave's 64 lanes read 64 neighbouring channels of one row; 4 cw items over 1024 threads (cw = 768: three per thread)
    const int count = ntok - 1;
    const int cw = dim / S, c0 = slice * cw;
    const int items = 4 * cw;
    for (int it = tid; it < items; it += kTapThreads) {
        const int grp = it / cw, lc = it - grp * cw;
        const float gc = g[c0 + lc], bc = b[c0 + lc];
        const float* xc = xb + dim + c0 + lc;   // the channel in the first patch row
        float s = 0.f, m = -INFINITY;
#pragma unroll 4
        for (int p = grp; p < count; p += 4) {
            const float2 st = s_row[1 + p];
            const float v = fmaf((xc[(int64_t)p * dim] - st.x) * st.y, gc, bc);
            s += v;
            m = fmaxf(m, v);
        }
        s_sum[grp][lc] = s;   // (an empty group, count < 4: 0 and -inf)
        s_max[grp][lc] = m;
    }
    __syncthreads();
    float* o = pooled_out + n * 3 * dim + c0;
    if (tid < cw) {
        const float mean = ((s_sum[0][tid] + s_sum[1][tid]) + (s_sum[2][tid] + s_sum[3][tid])) / (float)count;
        s_mean[tid] = mean;
        o[tid] = mean;
        o[dim + tid] = fmaxf(fmaxf(s_max[0][tid], s_max[1][tid]), fmaxf(s_max[2][tid], s_max[3][tid]));
    }
    __syncthreads();
    for (int it = tid; it < items; it += kTapThreads) {
        const int grp = it / cw, lc = it - grp * cw;
        const float gc = g[c0 + lc], bc = b[c0 + lc], mean = s_mean[lc];
        const float* xc = xb + dim + c0 + lc;
        float q = 0.f;
#pragma unroll 4
        for (int p = grp; p < count; p += 4) {
            const float2 st = s_row[1 + p];
            const float dv = fmaf((xc[(int64_t)p * dim] - st.x) * st.y, gc, bc) - mean;
            q = fmaf(dv, dv, q);
        }
        s_sum[grp][lc] = q;   // (every read of the sums is behind the barrier above)
    }
    __syncthreads();
    if (tid < cw) {
        const float var = ((s_sum[0][tid] + s_sum[1][tid]) + (s_sum[2][tid] + s_sum[3][tid])) / (float)count;
        o[2 * dim + tid] = sqrtf(var);
    }
}

// the slices of an image: the fewest that give the card kTapTargetGroups workgroups, a divisor of dim / 64 (a wave's 64 lanes stay in one token
// group), at most kTapMaxSlices
static int tap_slices(int Nimg, int dim) {
    int best = 1;
    for (int d = 1; d <= kTapMaxSlices; ++d) {
        if ((dim / 64) % d) continue;
        best = d;
        if ((int64_t)Nimg * d >= kTapTargetGroups) break;
    }
    return best;
}

int launch_vit_norm_token_stats(relax_handle* h, const float* X, const float* g, const float* b, float eps, float* cls_out, float* pooled_out,
                                int Nimg, int ntok, int dim, hipStream_t s) {
    RELAX_REQUIRE(h, dim % 64 == 0 && dim > 0 && dim <= kTapMaxDim, "vit_norm_token_stats: dim=%d must be a multiple of 64, <= %d", dim, kTapMaxDim);
    RELAX_REQUIRE(h, ntok >= 2 && ntok <= kTapMaxTok, "vit_norm_token_stats: ntok=%d outside [2, %d]", ntok, kTapMaxTok);
    RELAX_REQUIRE(h, X && g && b && Nimg > 0 && (cls_out || pooled_out), "vit_norm_token_stats: bad arguments");
    const int S = pooled_out ? tap_slices(Nimg, dim) : 1;
    const int64_t groups = (int64_t)8 * S * ((Nimg + 7) / 8);
    RELAX_REQUIRE(h, groups <= INT32_MAX, "vit_norm_token_stats: %d images", Nimg);
    hipLaunchKernelGGL(vit_norm_token_stats, dim3((unsigned)groups), dim3(kTapThreads), 0, s, X, g, b, eps, cls_out, pooled_out, Nimg, dim, ntok, S);
    RELAX_HIP_CHECK(h, hipGetLastError());
    return RELAX_OK;
}

}  // namespace relax

extern "C" int relax_op_vit_norm_token_stats(relax_handle* h, const float* x, const float* gamma, const float* beta, float eps, float* cls_out,
                                             float* pooled_out, int Nimg, int ntok, int dim, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    return relax::launch_vit_norm_token_stats(h, x, gamma, beta, eps, cls_out, pooled_out, Nimg, ntok, dim, static_cast<hipStream_t>(stream));
}
