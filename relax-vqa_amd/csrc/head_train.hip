// Training of the quality head on the device: scaler fit, one SGD or Adam / AdamW step of the reference's Mlp
// under its MAE + rank criterion, evaluation, the SWA average, the BatchNorm refresh, import / export.
//   src/model_regression.py:122-135  preprocess_data: NaN / inf -> 0, SimpleImputer(mean).fit, MinMaxScaler.fit / transform
//   src/model_regression.py:37-58    Mlp (train mode: BatchNorm1d on batch statistics, dropout)
//   src/model_regression.py:69-89    MAEAndRankLoss.forward (use_margin off)
//   src/model_regression.py:292-322  train_one_epoch / evaluate
//   src/model_regression.py:381-389  optim.SGD(momentum=0.9) | optim.Adam, AveragedModel;  :459 torch.optim.swa_utils.update_bn
//   src/fine_tune.py:151-155         optim.AdamW
//   src/model_regression_simple.py:37-58   the plain Mlp (bn1 commented out): a state made by relax_head_train_init_ex(batchnorm = 0)
// Everything of a step is enqueued on the caller's stream; nothing here waits for the device except the entries that
// say so (init, import, export, loss_read).  All arithmetic is fp32 with fp32 accumulation (fc1 / fc2 forward on the
// exact-fp32 contraction of gemm.hip whatever "gemm_precision" is set: ht_gemm).
//
// The batch rows are gathered into a contiguous [B][Fpad] block once per step (ht_gather): the fc1 contraction and the
// dW1 kernel both read that block.  Its cost is one read and one write of the batch per step (72 MB at F = 35203,
// B = 256) - over an epoch exactly what a per-epoch permuted copy of the matrix would move, without a second matrix.
//
// Dropout: a counter-based generator (a 64-bit mix of seed, step, layer, element) - no state, the same mask for the same
// key.  It does not and cannot reproduce torch's Philox stream; a step can write out the masks it used instead.
#include <cmath>
#include <cstring>

#include "relax_internal.h"
#include "host_logic.h"
#include "gelu.h"

namespace relax {

namespace {

constexpr float kBnEps = 1e-5f;
constexpr float kBnMomentum = 0.1f;

// offsets (in floats) of the tensors of one parameter set
struct HtLayout {
    size_t w1, b1, gamma, beta, w2, b2, w3, b3, rmean, rvar, n_params, n_all;
};

// batchnorm == false: the plain head - the four bn1 blocks are empty (their offsets are never used), n_all == n_params
HtLayout ht_layout(int Fpad, int H1, int H2, bool batchnorm) {
    HtLayout L{};
    const size_t bn = batchnorm ? (size_t)H1 : 0;
    size_t o = 0;
    L.w1 = o; o += (size_t)H1 * Fpad;
    L.b1 = o; o += H1;
    L.gamma = o; o += bn;
    L.beta = o; o += bn;
    L.w2 = o; o += (size_t)H2 * H1;
    L.b2 = o; o += H2;
    L.w3 = o; o += H2;
    L.b3 = o; o += 4;   // one float, padded: rmean stays 16-byte aligned
    L.n_params = o;
    L.rmean = o; o += bn;
    L.rvar = o; o += bn;
    L.n_all = o;
    return L;
}

// activations of one batch, in floats, for a batch capacity of mb rows
struct HtAct {
    size_t z1, xhat, a1, du1, dz1, z2, a2, dz2, p, yb, dp, rowloss, invstd, total;
};

HtAct ht_act(int mb, int H1, int H2) {
    HtAct A{};
    size_t o = 0;
    auto take = [&](size_t n) { size_t r = o; o += (n + 3) / 4 * 4; return r; };
    A.z1 = take((size_t)mb * H1); A.xhat = take((size_t)mb * H1); A.a1 = take((size_t)mb * H1);
    A.du1 = take((size_t)mb * H1); A.dz1 = take((size_t)mb * H1);
    A.z2 = take((size_t)mb * H2); A.a2 = take((size_t)mb * H2); A.dz2 = take((size_t)mb * H2);
    A.p = take(mb); A.yb = take(mb); A.dp = take(mb); A.rowloss = take(mb); A.invstd = take(H1);
    A.total = o;
    return A;
}

__device__ inline uint64_t ht_mix64(uint64_t x) {   // the splitmix64 finaliser
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// 32 uniform bits for the key (seed, step, layer, element)
__device__ inline uint32_t ht_rand(uint64_t seed, uint64_t step, uint32_t layer, uint64_t elem) {
    uint64_t k = ht_mix64(seed + 0x9E3779B97F4A7C15ull * (step + 1));
    k = ht_mix64(k ^ (0xD1B54A32D192ED03ull * (uint64_t)(layer + 1)));
    return (uint32_t)(ht_mix64(k + 0x9E3779B97F4A7C15ull * elem) >> 32);
}

struct HtDrop {
    uint64_t seed, step;
    uint32_t threshold;   // an element is dropped when its 32 bits are below this: drop_rate * 2^32
    float scale;          // 1 / (1 - drop_rate)
};

// sum over the block's 256 threads, in one fixed tree order (the result does not depend on scheduling); all threads get it
__device__ inline float ht_block_sum(float v, float* sh) {
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) sh[t] += sh[t + s];
        __syncthreads();
    }
    return sh[0];
}

}  // namespace

// ---- scaler fit --------------------------------------------------------------------------------------------------------
// pass 1: thread = one column, rows blockIdx.y, blockIdx.y + gridDim.y, ...: coalesced along F, the matrix is read once
__global__ __launch_bounds__(256) void ht_scaler_partial(const float* __restrict__ x, int n, int F, double* __restrict__ psum,
                                                         float* __restrict__ pmin, float* __restrict__ pmax) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    double s = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    for (int r = blockIdx.y; r < n; r += gridDim.y) {
        float v = x[(int64_t)r * F + f];
        if (!(fabsf(v) <= 3.402823466e38f)) v = 0.f;   // NaN, +inf, -inf -> 0
        s += (double)v;
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    const int64_t o = (int64_t)blockIdx.y * F + f;
    psum[o] = s;
    pmin[o] = mn;
    pmax[o] = mx;
}

// pass 2: the row groups of a column in order; SimpleImputer.statistics_, MinMaxScaler.scale_ / .min_ (sklearn's
// _handle_zeros_in_scale: a range below 10 eps(float64) scales by 1)
__global__ __launch_bounds__(256) void ht_scaler_finish(const double* __restrict__ psum, const float* __restrict__ pmin,
                                                        const float* __restrict__ pmax, int groups, int n, int F,
                                                        double* __restrict__ stats, double* __restrict__ scale,
                                                        double* __restrict__ mn_out, double* __restrict__ dmin_out,
                                                        double* __restrict__ dmax_out) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    double s = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    for (int g = 0; g < groups; ++g) {
        const int64_t o = (int64_t)g * F + f;
        s += psum[o];
        mn = fminf(mn, pmin[o]);
        mx = fmaxf(mx, pmax[o]);
    }
    const double dmin = (double)mn, dmax = (double)mx;
    const double range = dmax - dmin;
    const double sc = range < 10.0 * 2.220446049250313e-16 ? 1.0 : 1.0 / range;
    stats[f] = s / (double)n;
    scale[f] = sc;
    mn_out[f] = 0.0 - dmin * sc;
    if (dmin_out) dmin_out[f] = dmin;
    if (dmax_out) dmax_out[f] = dmax;
}

// the training transform: NaN / inf -> 0, then (double) x * scale + min -> float, K zero padded to Fpad
// (head_preprocess of head.hip, which the inference head keeps, substitutes the column mean for NaN and leaves inf)
__global__ __launch_bounds__(256) void ht_preprocess(const float* __restrict__ x, const double* __restrict__ scale,
                                                     const double* __restrict__ mn, float* __restrict__ xp, int F, int Fpad,
                                                     int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int f = (int)(i % Fpad);
    const int64_t r = i / Fpad;
    float o = 0.f;
    if (f < F) {
#pragma clang fp contract(off)   // two roundings, as numpy's X * scale_ + min_ (no fused multiply-add)
        float v = x[r * F + f];
        if (!(fabsf(v) <= 3.402823466e38f)) v = 0.f;
        const double prod = (double)v * scale[f];
        o = (float)(prod + mn[f]);
    }
    xp[i] = o;
}

// ---- forward -----------------------------------------------------------------------------------------------------------
// xb[b] = xp[idx[b]] (16-byte copies), yb[b] = y[idx[b]]; tick: num_batches_tracked += 1 (one thread)
__global__ __launch_bounds__(256) void ht_gather(const float* __restrict__ xp, const float* __restrict__ y, const int32_t* __restrict__ idx,
                                                 int n, int Fpad, float* __restrict__ xb, float* __restrict__ yb, int64_t* nbt) {
    const int b = blockIdx.x;
    int r = idx[b];
    r = r < 0 ? 0 : (r >= n ? n - 1 : r);   // the list is device memory and no entry reads it: a row outside [0, n) is CLAMPED (the step then
                                            // trains on a wrong row, silently) so that nothing is ever read outside the matrix; HeadTrainer checks host lists
    const float4* src = reinterpret_cast<const float4*>(xp + (int64_t)r * Fpad);
    float4* dst = reinterpret_cast<float4*>(xb + (int64_t)b * Fpad);
    const int q = Fpad / 4;
    for (int i = blockIdx.y * blockDim.x + threadIdx.x; i < q; i += gridDim.y * blockDim.x) dst[i] = src[i];
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        if (y) yb[b] = y[r];
        if (b == 0 && nbt) *nbt += 1;
    }
}

// BatchNorm1d in train mode, one block per column: batch mean and biased variance, xhat, running statistics (unbiased
// variance; momentum 0.1, or 1 / num_batches_tracked when `cumulative` - torch's momentum=None of update_bn), then
// gamma * xhat + beta -> GELU -> inverted dropout.  With a1 == nullptr only the statistics are updated.
__global__ __launch_bounds__(256) void ht_bn_fwd(const float* __restrict__ z1, int B, int H1, const float* __restrict__ gamma,
                                                 const float* __restrict__ beta, float* __restrict__ rmean, float* __restrict__ rvar,
                                                 const int64_t* __restrict__ nbt, int cumulative, float* __restrict__ xhat,
                                                 float* __restrict__ invstd_out, float* __restrict__ a1, HtDrop drop,
                                                 uint8_t* __restrict__ mask_out) {
    __shared__ float sh[256];
    const int j = blockIdx.x;
    float s = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) s += z1[(int64_t)b * H1 + j];
    const float mean = ht_block_sum(s, sh) / (float)B;
    float q = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) {
        const float d = z1[(int64_t)b * H1 + j] - mean;
        q = fmaf(d, d, q);
    }
    const float ss = ht_block_sum(q, sh);
    const float var = ss / (float)B;
    const float invstd = 1.0f / sqrtf(var + kBnEps);
    if (threadIdx.x == 0) {
        const float m = cumulative ? 1.0f / (float)(*nbt) : kBnMomentum;
        rmean[j] = (1.0f - m) * rmean[j] + m * mean;
        rvar[j] = (1.0f - m) * rvar[j] + m * (ss / (float)(B - 1));
        if (invstd_out) invstd_out[j] = invstd;
    }
    if (!a1) return;
    const float g = gamma[j], be = beta[j];
    for (int b = threadIdx.x; b < B; b += 256) {
        const int64_t e = (int64_t)b * H1 + j;
        const float xh = (z1[e] - mean) * invstd;
        xhat[e] = xh;
        const bool keep = ht_rand(drop.seed, drop.step, 0, (uint64_t)e) >= drop.threshold;
        a1[e] = keep ? gelu_erf(fmaf(g, xh, be)) * drop.scale : 0.f;
        if (mask_out) mask_out[e] = keep ? 1 : 0;
    }
}

// BatchNorm1d in eval mode + GELU, element-wise
__global__ __launch_bounds__(256) void ht_bn_eval(const float* __restrict__ z1, int64_t total, int H1, const float* __restrict__ gamma,
                                                  const float* __restrict__ beta, const float* __restrict__ rmean,
                                                  const float* __restrict__ rvar, float* __restrict__ a1) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int j = (int)(e % H1);
    const float xh = (z1[e] - rmean[j]) / sqrtf(rvar[j] + kBnEps);
    a1[e] = gelu_erf(fmaf(gamma[j], xh, beta[j]));
}

// The plain head (no bn1) in train mode: a1 = dropout(GELU(z1)), four elements per thread (B * H1 is a multiple of four).  The key of
// an element is ht_bn_fwd's - (seed, step, layer 0, e) - so one (seed, step) gives both variants the same mask.
__global__ __launch_bounds__(256) void ht_plain_fwd(const float* __restrict__ z1, int64_t total4, float* __restrict__ a1, HtDrop drop,
                                                    uint8_t* __restrict__ mask_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total4) return;
    const float4 z = reinterpret_cast<const float4*>(z1)[i];
    const float zv[4] = {z.x, z.y, z.z, z.w};
    float av[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const bool keep = ht_rand(drop.seed, drop.step, 0, (uint64_t)(4 * i + c)) >= drop.threshold;
        av[c] = keep ? gelu_erf(zv[c]) * drop.scale : 0.f;
        if (mask_out) mask_out[4 * i + c] = keep ? 1 : 0;   // bytes: the caller's mask need not be 4-byte aligned
    }
    reinterpret_cast<float4*>(a1)[i] = make_float4(av[0], av[1], av[2], av[3]);
}

// one block per row: a2 = dropout(GELU(z2)) (train) or a2 = z2 as the contraction's GELU epilogue left it (eval); p = a2 . w3 + b3
__global__ __launch_bounds__(256) void ht_fwd_tail(const float* __restrict__ z2, int H2, const float* __restrict__ w3,
                                                   const float* __restrict__ b3, int train, float* __restrict__ a2,
                                                   float* __restrict__ p, HtDrop drop, uint8_t* __restrict__ mask_out) {
    __shared__ float sh[256];
    const int b = blockIdx.x;
    float s = 0.f;
    for (int k = threadIdx.x; k < H2; k += 256) {
        const int64_t e = (int64_t)b * H2 + k;
        float a = z2[e];
        if (train) {
            const bool keep = ht_rand(drop.seed, drop.step, 1, (uint64_t)e) >= drop.threshold;
            a = keep ? gelu_erf(a) * drop.scale : 0.f;
            a2[e] = a;
            if (mask_out) mask_out[e] = keep ? 1 : 0;
        }
        s = fmaf(a, w3[k], s);
    }
    s = ht_block_sum(s, sh);
    if (threadIdx.x == 0) p[b] = s + b3[0];
}

// ---- criterion ---------------------------------------------------------------------------------------------------------
// MAEAndRankLoss and its gradient, one block per row i of the B x B pair matrix:
//   loss = l1_w mean|p - y| + rank_w sum_ij relu(td_ij - sign(td_ij) pd_ij) / (B (B - 1)),   td = y_i - y_j, pd = p_i - p_j
// row i sums its own terms; p_i also sits in the terms (j, i) of the other rows, -td_ij - sign(td_ij) pd_ij, whose derivative with
// respect to p_i is -sign(td_ij) as well: both are evaluated here, so no second pass over the matrix is needed.
// sign(0) = 0 (a tied pair gives relu(0) = 0 and no gradient), relu'(0) = 0, as torch.  B = 1 has no pairs: the rank
// term is 0 there (the reference divides 0 by 0).
__global__ __launch_bounds__(256) void ht_criterion(const float* __restrict__ p, const float* __restrict__ y, int B, float l1_w,
                                                    float rank_w, float* __restrict__ rowloss, float* __restrict__ dp) {
    __shared__ float sh[256];
    const int i = blockIdx.x;
    const float pi = p[i], yi = y[i];
    float sum = 0.f, g = 0.f;
    for (int j = threadIdx.x; j < B; j += 256) {
        const float td = yi - y[j];
        const float sg = td > 0.f ? 1.f : (td < 0.f ? -1.f : 0.f);
        const float spd = sg * (pi - p[j]);
        const float v = td - spd;      // the pair (i, j)
        const float vt = -td - spd;    // the pair (j, i): td, sign and pd all change sign
        if (v > 0.f) {
            sum += v;
            g -= sg;
        }
        if (vt > 0.f) g -= sg;
    }
    sum = ht_block_sum(sum, sh);
    g = ht_block_sum(g, sh);
    if (threadIdx.x == 0) {
        const float pairs = (float)B * (float)(B - 1);
        const float rw = B > 1 ? rank_w / pairs : 0.f;
        const float d = pi - yi;
        const float sd = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
        rowloss[i] = l1_w * fabsf(d) / (float)B + rw * sum;
        if (dp) dp[i] = l1_w * sd / (float)B + rw * g;
    }
}

// batch loss = sum of the row terms in a fixed order; acc += {loss, loss * B, 1}  (train_one_epoch / evaluate weight a batch by its size)
__global__ __launch_bounds__(256) void ht_loss_finish(const float* __restrict__ rowloss, int B, double* __restrict__ acc,
                                                      float* __restrict__ loss_out) {
    __shared__ float sh[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < B; i += 256) s += rowloss[i];
    s = ht_block_sum(s, sh);
    if (threadIdx.x == 0) {
        if (acc) {
            acc[0] += (double)s;
            acc[1] += (double)s * (double)B;
            acc[2] += 1.0;
        }
        if (loss_out) *loss_out = s;
    }
}

// ---- backward ----------------------------------------------------------------------------------------------------------
// dz2 = dp w3 * mask2 / (1 - rate) * GELU'(z2)
__global__ __launch_bounds__(256) void ht_bwd_z2(const float* __restrict__ dp, const float* __restrict__ w3, const float* __restrict__ z2,
                                                 int64_t total, int H2, HtDrop drop, float* __restrict__ dz2) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int k = (int)(e % H2);
    const int64_t b = e / H2;
    const bool keep = ht_rand(drop.seed, drop.step, 1, (uint64_t)e) >= drop.threshold;
    dz2[e] = keep ? dp[b] * w3[k] * drop.scale * gelu_erf_grad(z2[e]) : 0.f;
}

// du1 = (dz2 W2) * mask1 / (1 - rate) * GELU'(gamma xhat + beta)
__global__ __launch_bounds__(256) void ht_bwd_u1(const float* __restrict__ dz2, const float* __restrict__ w2, const float* __restrict__ xhat,
                                                 const float* __restrict__ gamma, const float* __restrict__ beta, int64_t total, int H1,
                                                 int H2, HtDrop drop, float* __restrict__ du1) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int j = (int)(e % H1);
    const int64_t b = e / H1;
    float s = 0.f;
    for (int k = 0; k < H2; ++k) s = fmaf(dz2[b * H2 + k], w2[(int64_t)k * H1 + j], s);
    const bool keep = ht_rand(drop.seed, drop.step, 0, (uint64_t)e) >= drop.threshold;
    du1[e] = keep ? s * drop.scale * gelu_erf_grad(fmaf(gamma[j], xhat[e], beta[j])) : 0.f;
}

struct HtSgd {
    float lr, mu, wd;
};

__device__ inline void ht_sgd(float& w, float& m, float grad, const HtSgd o) {   // torch SGD(momentum, dampening 0, no nesterov)
    const float g = fmaf(o.wd, w, grad);
    m = fmaf(o.mu, m, g);
    w = fmaf(-o.lr, m, w);
}

// torch's Adam (wd: g = grad + wd w) or AdamW (decay = 1 - lr wd: w *= decay, then g = grad) for step t.  The bias corrections come
// from the host, in double from t: step_size = lr / (1 - b1^t), inv_sqrt_bc2 = 1 / sqrt(1 - b2^t).  The form not in use is inert:
// decay = 1 under Adam and wd = 0 under AdamW are both exact.
struct HtAdam {
    float b1, omb1, b2, omb2, eps, wd, decay, step_size, inv_sqrt_bc2;   // omb = 1 - b, rounded once from the double
};

__device__ inline void ht_adam(float& w, float& m, float& v, float grad, const HtAdam o) {
    w *= o.decay;
    const float g = fmaf(o.wd, w, grad);
    m = fmaf(o.b1, m, o.omb1 * g);
    v = fmaf(o.b2, v, o.omb2 * g * g);
    w = fmaf(-o.step_size, m / fmaf(sqrtf(v), o.inv_sqrt_bc2, o.eps), w);   // g = 0 on m = v = 0 (the K padding): 0 / eps = 0
}

// Parameter i (or the float4 of them at i) under either optimizer: `m` is the momentum buffer / exp_avg, `v` exp_avg_sq, which SGD
// never touches (it may be null there)
__device__ inline void ht_update(float* w, float* m, float*, int64_t i, float grad, const HtSgd o) { ht_sgd(w[i], m[i], grad, o); }
__device__ inline void ht_update(float* w, float* m, float* v, int64_t i, float grad, const HtAdam o) { ht_adam(w[i], m[i], v[i], grad, o); }

__device__ inline void ht_update4(float* w1, float* m1, float*, int64_t i, const float4 g, const HtSgd o) {
    float4 *wp = reinterpret_cast<float4*>(w1 + i), *mp = reinterpret_cast<float4*>(m1 + i);
    float4 w = *wp, m = *mp;
    ht_sgd(w.x, m.x, g.x, o);
    ht_sgd(w.y, m.y, g.y, o);
    ht_sgd(w.z, m.z, g.z, o);
    ht_sgd(w.w, m.w, g.w, o);
    *wp = w;
    *mp = m;
}

__device__ inline void ht_update4(float* w1, float* m1, float* v1, int64_t i, const float4 g, const HtAdam o) {
    float4 *wp = reinterpret_cast<float4*>(w1 + i), *mp = reinterpret_cast<float4*>(m1 + i), *vp = reinterpret_cast<float4*>(v1 + i);
    float4 w = *wp, m = *mp, v = *vp;
    ht_adam(w.x, m.x, v.x, g.x, o);
    ht_adam(w.y, m.y, v.y, g.y, o);
    ht_adam(w.z, m.z, v.z, g.z, o);
    ht_adam(w.w, m.w, v.w, g.w, o);
    *wp = w;
    *mp = m;
    *vp = v;
}

// BatchNorm backward, one block per column: dgamma, dbeta, dz1 = gamma invstd (du1 - mean(du1) - xhat mean(du1 xhat)), db1 = sum dz1
// (zero but for rounding: a bias in front of a BatchNorm has no gradient), and the optimizer's update of gamma, beta, fc1.bias
// (m_*: momentum buffer / exp_avg, v_*: exp_avg_sq, null under SGD)
template <class Opt>
__global__ __launch_bounds__(256) void ht_bn_bwd(const float* __restrict__ du1, const float* __restrict__ xhat, const float* __restrict__ invstd,
                                                 int B, int H1, float* __restrict__ gamma, float* __restrict__ beta, float* __restrict__ b1,
                                                 float* __restrict__ m_gamma, float* __restrict__ m_beta, float* __restrict__ m_b1,
                                                 float* __restrict__ v_gamma, float* __restrict__ v_beta, float* __restrict__ v_b1,
                                                 Opt opt, float* __restrict__ dz1) {
    __shared__ float sh[256];
    const int j = blockIdx.x;
    float s = 0.f, sx = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) {
        const int64_t e = (int64_t)b * H1 + j;
        s += du1[e];
        sx = fmaf(du1[e], xhat[e], sx);
    }
    const float dbeta = ht_block_sum(s, sh);
    const float dgamma = ht_block_sum(sx, sh);
    const float c = gamma[j] * invstd[j];
    const float mb = dbeta / (float)B, mg = dgamma / (float)B;
    float sz = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) {
        const int64_t e = (int64_t)b * H1 + j;
        const float d = c * (du1[e] - mb - xhat[e] * mg);
        dz1[e] = d;
        sz += d;
    }
    const float db1 = ht_block_sum(sz, sh);   // (also the barrier between every thread's read of gamma[j] and its update)
    if (threadIdx.x == 0) {
        ht_update(gamma, m_gamma, v_gamma, j, dgamma, opt);
        ht_update(beta, m_beta, v_beta, j, dbeta, opt);
        ht_update(b1, m_b1, v_b1, j, db1, opt);
    }
}

// The plain head's backward through fc2 and the first activation, and fc1.bias - which has a real gradient here - in one launch:
//   dz1[b,j] = keep ? (sum_k dz2[b,k] W2[k,j]) * scale * GELU'(z1[b,j]) : 0     k ascending with fmaf, ht_bwd_u1's order
//   db1[j]   = sum_b dz1[b,j], then the optimizer's update of fc1.bias[j]
// A block owns kPbJ = 4 columns j and all B rows: thread (ty, tx) takes column j0 + tx and the rows ty, ty + 64, ... in ascending order;
// its partial column sum goes to LDS and thread (0, tx) adds the 64 partials in the order of ty.  Nothing atomic, no order that
// depends on the launch: the same bits on every run.  Runs before ht_update_small, which changes W2.
constexpr int kPbJ = 4, kPbRows = 256 / kPbJ;

template <class Opt>
__global__ __launch_bounds__(256) void ht_plain_bwd(const float* __restrict__ dz2, const float* __restrict__ w2, const float* __restrict__ z1,
                                                    int B, int H1, int H2, HtDrop drop, float* __restrict__ b1, float* __restrict__ m_b1,
                                                    float* __restrict__ v_b1, Opt opt, float* __restrict__ dz1) {
    __shared__ float part[kPbRows][kPbJ];
    const int tx = threadIdx.x & (kPbJ - 1), ty = threadIdx.x / kPbJ;
    const int j = blockIdx.x * kPbJ + tx;   // H1 % 128 == 0: always a column
    float colsum = 0.f;
    for (int b = ty; b < B; b += kPbRows) {
        const float4* row = reinterpret_cast<const float4*>(dz2 + (int64_t)b * H2);   // H2 % 64 == 0 and dz2 is 16-byte aligned
        float s = 0.f;
        for (int k4 = 0; k4 < H2 / 4; ++k4) {
            const float4 d = row[k4];
            const float* w = w2 + (int64_t)(4 * k4) * H1 + j;
            s = fmaf(d.x, w[0], s);
            s = fmaf(d.y, w[H1], s);
            s = fmaf(d.z, w[2 * (int64_t)H1], s);
            s = fmaf(d.w, w[3 * (int64_t)H1], s);
        }
        const int64_t e = (int64_t)b * H1 + j;
        const bool keep = ht_rand(drop.seed, drop.step, 0, (uint64_t)e) >= drop.threshold;
        const float d1 = keep ? s * drop.scale * gelu_erf_grad(z1[e]) : 0.f;
        dz1[e] = d1;
        colsum += d1;
    }
    part[ty][tx] = colsum;
    __syncthreads();
    if (ty == 0) {
        float db1 = 0.f;
        for (int r = 0; r < kPbRows; ++r) db1 += part[r][tx];
        ht_update(b1, m_b1, v_b1, j, db1, opt);
    }
}

// fc2.weight (dW2 = dz2^T a1), fc2.bias, fc3.weight, fc3.bias: gradient and the optimizer's update, one thread per parameter.  These
// four tensors are contiguous in the set (W2 | b2 | w3 | b3), `par` / `mom` / `var` point at W2.
template <class Opt>
__global__ __launch_bounds__(256) void ht_update_small(const float* __restrict__ dz2, const float* __restrict__ a1, const float* __restrict__ a2,
                                                       const float* __restrict__ dp, int B, int H1, int H2, float* __restrict__ par,
                                                       float* __restrict__ mom, float* __restrict__ var, Opt opt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int nw2 = H2 * H1;
    if (i >= nw2 + 2 * H2 + 1) return;
    float g = 0.f;
    if (i < nw2) {
        const int k = i / H1, j = i % H1;
        for (int b = 0; b < B; ++b) g = fmaf(dz2[(int64_t)b * H2 + k], a1[(int64_t)b * H1 + j], g);
    } else if (i < nw2 + H2) {
        const int k = i - nw2;
        for (int b = 0; b < B; ++b) g += dz2[(int64_t)b * H2 + k];
    } else if (i < nw2 + 2 * H2) {
        const int k = i - nw2 - H2;
        for (int b = 0; b < B; ++b) g = fmaf(dp[b], a2[(int64_t)b * H2 + k], g);
    } else {
        for (int b = 0; b < B; ++b) g += dp[b];
    }
    ht_update(par, mom, var, i, g, opt);
}

// The hot kernel: dW1 = dz1^T X_b ([H1][Fpad], contracted over the B rows of the batch) with the optimizer's update in its epilogue -
// the gradient of fc1.weight is never written; a tile of W1 and of its momentum (Adam: of both moments) is read and written once.
// 64 (j) x 128 (f) tile per workgroup of 256 threads, 4 x 8 accumulators per thread in fp32, 16 batch rows per LDS stage.
// Both operands have the contraction index as their slow one (dz1 [B][H1], X_b [B][Fpad]), so a stage is plain 16-byte
// row loads.  Columns f >= F are zero in X_b and in W1, and stay exactly zero (SGD: g = 0 + wd * 0; Adam: 0 / (0 + eps)).
constexpr int kDwTJ = 64, kDwTF = 128, kDwKB = 16;

// kFused = false (tools/head_train_bench.py only): the same tiles write dW1 to `grad` and ht_apply updates in a second pass.
template <bool kFused, class Opt>
__device__ __forceinline__ void ht_dw1(const float* __restrict__ dz1, const float* __restrict__ xb, int B, int H1, int Fpad,
                                       float* __restrict__ w1, float* __restrict__ m1, float* __restrict__ v1, Opt opt,
                                       float* __restrict__ grad) {
    __shared__ float4 As[kDwKB][kDwTJ / 4];
    __shared__ float4 Xs[kDwKB][kDwTF / 4];
    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;
    const int j0 = blockIdx.x * kDwTJ;
    const int f0 = blockIdx.y * kDwTF;
    float acc[4][8];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[a][c] = 0.f;

    const int ar = tid >> 4, ac = tid & 15;    // dz1 stage: 16 rows x 16 float4
    const int xr = tid >> 5, xc = tid & 31;    // X_b stage: 2 x (8 rows x 32 float4)
    const bool x_in = f0 + xc * 4 < Fpad;      // Fpad % 4 == 0: a float4 is inside or outside as a whole
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int b0 = 0; b0 < B; b0 += kDwKB) {
        float4 av = zero, xv0 = zero, xv1 = zero;
        if (b0 + ar < B) av = *reinterpret_cast<const float4*>(dz1 + (int64_t)(b0 + ar) * H1 + j0 + ac * 4);
        if (x_in && b0 + xr < B) xv0 = *reinterpret_cast<const float4*>(xb + (int64_t)(b0 + xr) * Fpad + f0 + xc * 4);
        if (x_in && b0 + xr + 8 < B) xv1 = *reinterpret_cast<const float4*>(xb + (int64_t)(b0 + xr + 8) * Fpad + f0 + xc * 4);
        __syncthreads();   // the previous stage has been consumed
        As[ar][ac] = av;
        Xs[xr][xc] = xv0;
        Xs[xr + 8][xc] = xv1;
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kDwKB; ++kk) {
            const float4 a = As[kk][ty];
            const float4 x0 = Xs[kk][tx], x1 = Xs[kk][16 + tx];
            const float av4[4] = {a.x, a.y, a.z, a.w};
            const float xv8[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 8; ++c) acc[r][c] = fmaf(av4[r], xv8[c], acc[r][c]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int j = j0 + ty * 4 + r;   // H1 % 64 == 0: always a row of W1
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int f = f0 + half * 64 + tx * 4;
            if (f >= Fpad) continue;
            const float4 g = make_float4(acc[r][half * 4 + 0], acc[r][half * 4 + 1], acc[r][half * 4 + 2], acc[r][half * 4 + 3]);
            const int64_t o = (int64_t)j * Fpad + f;
            if (!kFused) {
                *reinterpret_cast<float4*>(grad + o) = g;
                continue;
            }
            ht_update4(w1, m1, v1, o, g, opt);
        }
    }
}

template <bool kFused>
__global__ __launch_bounds__(256) void ht_dw1_sgd(const float* __restrict__ dz1, const float* __restrict__ xb, int B, int H1, int Fpad,
                                                  float* __restrict__ w1, float* __restrict__ m1, HtSgd sgd, float* __restrict__ grad) {
    ht_dw1<kFused>(dz1, xb, B, H1, Fpad, w1, m1, (float*)nullptr, sgd, grad);
}

// the Adam form: 252 MB per step at F = 35203, H1 = B = 256 (X_b once, W1 and both moments read and written) against SGD's 180 MB
template <bool kFused>
__global__ __launch_bounds__(256) void ht_dw1_adam(const float* __restrict__ dz1, const float* __restrict__ xb, int B, int H1, int Fpad,
                                                   float* __restrict__ w1, float* __restrict__ m1, float* __restrict__ v1, HtAdam adam,
                                                   float* __restrict__ grad) {
    ht_dw1<kFused>(dz1, xb, B, H1, Fpad, w1, m1, v1, adam, grad);
}

// the separate update of the unfused form (ht_sgd_apply, ht_adam_apply): one float4 of W1, its optimizer state and the gradient per thread
template <class Opt>
__device__ __forceinline__ void ht_apply(const float* __restrict__ grad, float* __restrict__ w, float* __restrict__ m,
                                         float* __restrict__ v, int64_t n4, Opt opt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    ht_update4(w, m, v, 4 * i, reinterpret_cast<const float4*>(grad)[i], opt);
}

__global__ __launch_bounds__(256) void ht_sgd_apply(const float* __restrict__ grad, float* __restrict__ w, float* __restrict__ m, int64_t n4,
                                                    HtSgd sgd) {
    ht_apply(grad, w, m, (float*)nullptr, n4, sgd);
}

__global__ __launch_bounds__(256) void ht_adam_apply(const float* __restrict__ grad, float* __restrict__ w, float* __restrict__ m,
                                                     float* __restrict__ v, int64_t n4, HtAdam adam) {
    ht_apply(grad, w, m, v, n4, adam);
}

// ---- SWA ---------------------------------------------------------------------------------------------------------------
// AveragedModel.update_parameters over the parameter part of the set: the first call copies, then avg += (p - avg) / (n + 1)
__global__ __launch_bounds__(256) void ht_swa_update(const float* __restrict__ p, float* __restrict__ avg, int64_t total,
                                                     int64_t* __restrict__ n_averaged) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t n = *n_averaged;
    avg[i] = n == 0 ? p[i] : avg[i] + (p[i] - avg[i]) / (float)(n + 1);
}

__global__ void ht_count(int64_t* c, int64_t add) { *c += add; }

__global__ __launch_bounds__(256) void ht_bn_reset(float* __restrict__ rmean, float* __restrict__ rvar, int H1, int64_t* nbt) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < H1) {
        rmean[j] = 0.f;
        rvar[j] = 1.f;
    }
    if (j == 0) *nbt = 0;
}

void free_head_train(relax_handle* h) {
    HeadTrain& t = h->head_train;
    t.mem.release();
    if (t.scaler_ws.p) (void)hipFree(t.scaler_ws.p);
    t = HeadTrain();
}

namespace {

HtDrop make_drop(float rate, uint64_t seed, uint64_t step) {
    HtDrop d{};
    d.seed = seed;
    d.step = step;
    d.threshold = (uint32_t)((double)rate * 4294967296.0);
    d.scale = 1.0f / (1.0f - rate);
    return d;
}

struct HtItem {   // a tensor of a state dict and where it sits in a set
    const char* key;
    size_t off;
    int64_t numel;
};

// A plain state (no bn1) takes no bn1.* tensor: the first such key is refused by name ('module.' stripped as the loaders strip it)
int ht_refuse_bn_keys(relax_handle* h, const char* what, const char* const* names, int n) {
    for (int i = 0; i < n; ++i) {
        if (!names[i]) continue;
        std::string key(names[i]);
        if (key.rfind("module.", 0) == 0) key = key.substr(7);
        RELAX_REQUIRE(h, key.rfind("bn1.", 0) != 0, "%s: key '%s' into a state without BatchNorm (relax_head_train_init_ex, batchnorm 0)", what,
                      key.c_str());
    }
    return RELAX_OK;
}

int ht_check_batch(relax_handle* h, const char* what, const void* xp, const void* idx, int n, int B, int min_b) {
    const HeadTrain& t = h->head_train;
    RELAX_REQUIRE(h, t.ready, "%s: call relax_head_train_init first", what);
    RELAX_REQUIRE(h, xp && idx && n > 0, "%s: bad arguments", what);
    RELAX_REQUIRE(h, B >= min_b && B <= t.max_batch, "%s: batch of %d rows (this state takes %d..%d)", what, B, min_b, t.max_batch);
    RELAX_REQUIRE(h, (reinterpret_cast<uintptr_t>(xp) & 15) == 0, "%s: the matrix must be 16-byte aligned", what);
    return RELAX_OK;
}

// fc1 / fc2 on the exact-fp32 contraction whatever "gemm_precision" the handle carries (1 would route launch_conv to bf16x3)
int ht_gemm(relax_handle* h, const float* A, const float* W, const float* bias, float* out, int M, int N, int K, int act, hipStream_t s) {
    const int saved = h->gemm.precision;
    h->gemm.precision = 0;
    const int rc = launch_gemm(h, A, W, bias, nullptr, out, M, N, K, act, s);
    h->gemm.precision = saved;
    return rc;
}

dim3 gather_grid(int B, int Fpad) { return dim3((unsigned)B, (unsigned)std::min(8, (Fpad / 4 + 255) / 256)); }

// A block in a set's layout to HOST memory, in the order of the flat block below; `params_only`: the block is optimizer state, which has
// the parameter part alone - zeros go under the two buffer keys
int ht_export_block(relax_handle* h, const float* src, bool params_only, float* out) {
    const HeadTrain& t = h->head_train;
    const HtLayout L = ht_layout(t.Fpad, t.H1, t.H2, t.batchnorm);
    float* o = out;
    RELAX_HIP_CHECK(h, hipMemcpy2D(o, sizeof(float) * t.F, src + L.w1, sizeof(float) * t.Fpad, sizeof(float) * t.F, t.H1, hipMemcpyDeviceToHost));
    o += (size_t)t.H1 * t.F;
    auto put = [&](size_t off, size_t numel) -> hipError_t {
        hipError_t e = hipSuccess;
        if (params_only && off >= L.n_params) std::memset(o, 0, sizeof(float) * numel);
        else e = hipMemcpy(o, src + off, sizeof(float) * numel, hipMemcpyDeviceToHost);
        o += numel;
        return e;
    };
    // order of the flat block: fc1.weight [H1,F], fc1.bias, bn1.weight, bn1.bias, bn1.running_mean, bn1.running_var, fc2.weight, fc2.bias,
    // fc3.weight, fc3.bias; a plain state has no bn1 tensors and writes the other six
    RELAX_HIP_CHECK(h, put(L.b1, t.H1));
    if (t.batchnorm) {
        RELAX_HIP_CHECK(h, put(L.gamma, t.H1));
        RELAX_HIP_CHECK(h, put(L.beta, t.H1));
        RELAX_HIP_CHECK(h, put(L.rmean, t.H1));
        RELAX_HIP_CHECK(h, put(L.rvar, t.H1));
    }
    RELAX_HIP_CHECK(h, put(L.w2, (size_t)t.H2 * t.H1));
    RELAX_HIP_CHECK(h, put(L.b2, t.H2));
    RELAX_HIP_CHECK(h, put(L.w3, t.H2));
    RELAX_HIP_CHECK(h, put(L.b3, 1));
    return RELAX_OK;
}

// Adam's constants for step t (>= 1), every one computed in double as torch computes its Python scalars and rounded once
HtAdam make_adam(double lr, double beta1, double beta2, double eps, double weight_decay, int decoupled, int64_t t) {
    HtAdam a{};
    a.b1 = (float)beta1;
    a.omb1 = (float)(1.0 - beta1);
    a.b2 = (float)beta2;
    a.omb2 = (float)(1.0 - beta2);
    a.eps = (float)eps;
    a.wd = decoupled ? 0.f : (float)weight_decay;
    a.decay = decoupled ? (float)(1.0 - lr * weight_decay) : 1.f;
    a.step_size = (float)(lr / (1.0 - std::pow(beta1, (double)t)));
    a.inv_sqrt_bc2 = (float)(1.0 / std::sqrt(1.0 - std::pow(beta2, (double)t)));
    return a;
}

void launch_dw1(const HeadTrain& t, const float* dz1, int B, float* P, const HtSgd sgd, hipStream_t s) {
    hipLaunchKernelGGL(ht_dw1_sgd<true>, dim3((unsigned)(t.H1 / kDwTJ), (unsigned)((t.Fpad + kDwTF - 1) / kDwTF)), dim3(256), 0, s, dz1, t.xb,
                       B, t.H1, t.Fpad, P, t.mom, sgd, (float*)nullptr);
}

void launch_dw1(const HeadTrain& t, const float* dz1, int B, float* P, const HtAdam adam, hipStream_t s) {
    hipLaunchKernelGGL(ht_dw1_adam<true>, dim3((unsigned)(t.H1 / kDwTJ), (unsigned)((t.Fpad + kDwTF - 1) / kDwTF)), dim3(256), 0, s, dz1, t.xb,
                       B, t.H1, t.Fpad, P, t.mom, t.var, adam, (float*)nullptr);
}

// One iteration of train_one_epoch on the live set under either optimizer: the launches of a step, enqueued on `s`
template <class Opt>
int ht_step(relax_handle* h, const float* xp, const float* target, int n, const int32_t* index, int B, Opt opt, float l1_w,
            float rank_w, float drop_rate, uint64_t seed, uint64_t step, uint8_t* mask1, uint8_t* mask2, hipStream_t s) {
    HeadTrain& t = h->head_train;
    const int H1 = t.H1, H2 = t.H2, Fpad = t.Fpad;
    const HtLayout L = ht_layout(Fpad, H1, H2, t.batchnorm);
    const HtAct A = ht_act(t.max_batch, H1, H2);
    float* P = t.set[0];
    float* M = t.mom;
    float* V = t.var;   // SGD's kernels take it and leave it alone
    float* a = t.act;
    const HtDrop drop = make_drop(drop_rate, seed, step);
    const int64_t n1 = (int64_t)B * H1, n2 = (int64_t)B * H2;

    // a plain state has no num_batches_tracked to tick: counters[0] stays 0
    hipLaunchKernelGGL(ht_gather, gather_grid(B, Fpad), dim3(256), 0, s, xp, target, index, n, Fpad, t.xb, a + A.yb,
                       t.batchnorm ? t.counters + 0 : (int64_t*)nullptr);
    RELAX_TRY(ht_gemm(h, t.xb, P + L.w1, P + L.b1, a + A.z1, B, H1, Fpad, 0, s));
    if (t.batchnorm) {
        hipLaunchKernelGGL(ht_bn_fwd, dim3((unsigned)H1), dim3(256), 0, s, a + A.z1, B, H1, P + L.gamma, P + L.beta, P + L.rmean, P + L.rvar,
                           t.counters + 0, 0, a + A.xhat, a + A.invstd, a + A.a1, drop, mask1);
    } else {
        hipLaunchKernelGGL(ht_plain_fwd, dim3((unsigned)((n1 / 4 + 255) / 256)), dim3(256), 0, s, a + A.z1, n1 / 4, a + A.a1, drop, mask1);
    }
    RELAX_TRY(ht_gemm(h, a + A.a1, P + L.w2, P + L.b2, a + A.z2, B, H2, H1, 0, s));
    hipLaunchKernelGGL(ht_fwd_tail, dim3((unsigned)B), dim3(256), 0, s, a + A.z2, H2, P + L.w3, P + L.b3, 1, a + A.a2, a + A.p, drop, mask2);
    hipLaunchKernelGGL(ht_criterion, dim3((unsigned)B), dim3(256), 0, s, a + A.p, a + A.yb, B, l1_w, rank_w, a + A.rowloss, a + A.dp);
    hipLaunchKernelGGL(ht_loss_finish, dim3(1), dim3(256), 0, s, a + A.rowloss, B, t.loss, (float*)nullptr);
    hipLaunchKernelGGL(ht_bwd_z2, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, s, a + A.dp, P + L.w3, a + A.z2, n2, H2, drop, a + A.dz2);
    if (t.batchnorm) {
        hipLaunchKernelGGL(ht_bwd_u1, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, s, a + A.dz2, P + L.w2, a + A.xhat, P + L.gamma, P + L.beta,
                           n1, H1, H2, drop, a + A.du1);
        hipLaunchKernelGGL(ht_bn_bwd<Opt>, dim3((unsigned)H1), dim3(256), 0, s, a + A.du1, a + A.xhat, a + A.invstd, B, H1, P + L.gamma, P + L.beta,
                           P + L.b1, M + L.gamma, M + L.beta, M + L.b1, V + L.gamma, V + L.beta, V + L.b1, opt, a + A.dz1);
    } else {   // one launch where the BatchNorm step has two: a plain step makes one launch fewer
        hipLaunchKernelGGL(ht_plain_bwd<Opt>, dim3((unsigned)(H1 / kPbJ)), dim3(256), 0, s, a + A.dz2, P + L.w2, a + A.z1, B, H1, H2, drop,
                           P + L.b1, M + L.b1, V + L.b1, opt, a + A.dz1);
    }
    const int n_small = H2 * H1 + 2 * H2 + 1;
    hipLaunchKernelGGL(ht_update_small<Opt>, dim3((unsigned)((n_small + 255) / 256)), dim3(256), 0, s, a + A.dz2, a + A.a1, a + A.a2, a + A.dp, B,
                       H1, H2, P + L.w2, M + L.w2, V + L.w2, opt);
    launch_dw1(t, a + A.dz1, B, P + L.w1, opt, s);   // L.w1 == 0 in the optimizer's blocks too
    RELAX_HIP_CHECK(h, hipGetLastError());
    return RELAX_OK;
}

}  // namespace

}  // namespace relax

using namespace relax;

extern "C" {

int relax_head_fit_scaler(relax_handle* h, const float* x, int n, int F, double* imputer_statistics, double* scaler_scale,
                          double* scaler_min, double* data_min, double* data_max, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, x && n > 0 && F > 0 && imputer_statistics && scaler_scale && scaler_min, "relax_head_fit_scaler: bad arguments");
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int groups = std::max(1, std::min(32, (n + 15) / 16));
    const size_t per = (size_t)groups * F;
    RELAX_TRY(ensure_buf(h, h->head_train.scaler_ws, per * (sizeof(double) + 2 * sizeof(float))));
    double* psum = static_cast<double*>(h->head_train.scaler_ws.p);
    float* pmin = reinterpret_cast<float*>(psum + per);
    float* pmax = pmin + per;
    const unsigned cols = (unsigned)((F + 255) / 256);
    hipLaunchKernelGGL(ht_scaler_partial, dim3(cols, (unsigned)groups), dim3(256), 0, s, x, n, F, psum, pmin, pmax);
    hipLaunchKernelGGL(ht_scaler_finish, dim3(cols), dim3(256), 0, s, psum, pmin, pmax, groups, n, F, imputer_statistics, scaler_scale,
                       scaler_min, data_min, data_max);
    RELAX_HIP_CHECK(h, hipGetLastError());
    return RELAX_OK;
}

int relax_head_train_transform(relax_handle* h, const float* x, int n, int F, const double* scaler_scale, const double* scaler_min,
                               float* xp, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, x && xp && n > 0 && F > 0 && scaler_scale && scaler_min, "relax_head_train_transform: bad arguments");
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    const int Fpad = (F + 31) / 32 * 32;
    const int64_t total = (int64_t)n * Fpad;
    hipLaunchKernelGGL(ht_preprocess, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x,
                       scaler_scale, scaler_min, xp, F, Fpad, total);
    RELAX_HIP_CHECK(h, hipGetLastError());
    return RELAX_OK;
}

// relax_head_train_init and relax_head_train_init_ex; `what` names the entry in the messages
static int ht_init(relax_handle* h, const char* what, int input_features, int hidden_features, int max_batch, bool batchnorm) {
    RELAX_REQUIRE(h, input_features > 0 && hidden_features > 0, "%s: bad arguments", what);
    RELAX_REQUIRE(h, hidden_features % 128 == 0, "%s: hidden_features %d must be a multiple of 128 (fc2 is half of it, "
                  "and the contraction takes multiples of 64)", what, hidden_features);
    RELAX_REQUIRE(h, max_batch >= 2 && max_batch <= HeadTrain::kMaxBatch, "%s: max_batch %d outside 2..%d", what, max_batch,
                  HeadTrain::kMaxBatch);
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    RELAX_HIP_CHECK(h, hipDeviceSynchronize());
    free_head_train(h);
    HeadTrain& t = h->head_train;
    t.F = input_features;
    t.Fpad = (input_features + 31) / 32 * 32;
    t.H1 = hidden_features;
    t.H2 = hidden_features / 2;
    t.max_batch = max_batch;
    t.batchnorm = batchnorm;
    const HtLayout L = ht_layout(t.Fpad, t.H1, t.H2, t.batchnorm);
    t.n_params = L.n_params;
    t.n_all = L.n_all;
    int rc = RELAX_OK;
    auto grab = [&](size_t bytes) -> void* {
        if (rc != RELAX_OK) return nullptr;
        void* p = t.mem.keep(h, bytes, "relax_head_train_init's state");
        if (!p) {
            rc = RELAX_ERR_NOMEM;
            return nullptr;
        }
        if (hipMemset(p, 0, bytes) != hipSuccess) {
            set_error(h, "%s: hipMemset failed", what);
            rc = RELAX_ERR_HIP;
        }
        return p;
    };
    for (int i = 0; i < HeadTrain::kSets; ++i) t.set[i] = static_cast<float*>(grab(sizeof(float) * L.n_all));
    t.mom = static_cast<float*>(grab(sizeof(float) * L.n_params));
    t.var = static_cast<float*>(grab(sizeof(float) * L.n_params));
    t.counters = static_cast<int64_t*>(grab(sizeof(int64_t) * 2 * HeadTrain::kSets));
    t.loss = static_cast<double*>(grab(sizeof(double) * 6));
    t.act = static_cast<float*>(grab(sizeof(float) * ht_act(max_batch, t.H1, t.H2).total));
    t.xb = static_cast<float*>(grab(sizeof(float) * (size_t)max_batch * t.Fpad));
    // the contraction's tail split-K workspace: it asks for max(64 MiB, tail tiles x splits x 128 x 128 floats), and the tail fills the
    // chip at most once (768 work units of 64 KiB = 48 MiB): sized here, a step never finds it too small and so never waits for the device
    if (rc == RELAX_OK) rc = ensure_buf(h, h->splitk_ws, kSplitKWsFloor);
    if (rc == RELAX_OK && hipDeviceSynchronize() != hipSuccess) {   // the zero fills above have completed before anything is enqueued on another stream
        set_error(h, "%s: hipDeviceSynchronize failed", what);
        rc = RELAX_ERR_HIP;
    }
    if (rc != RELAX_OK) {
        free_head_train(h);
        return rc;
    }
    t.ready = true;
    return RELAX_OK;
}

int relax_head_train_init(relax_handle* h, int input_features, int hidden_features, int max_batch) {
    if (!h) return RELAX_ERR_INVALID;
    return ht_init(h, "relax_head_train_init", input_features, hidden_features, max_batch, true);
}

int relax_head_train_init_ex(relax_handle* h, int input_features, int hidden_features, int max_batch, int batchnorm) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, batchnorm == 0 || batchnorm == 1, "relax_head_train_init_ex: batchnorm %d (1: the Mlp with bn1, 0: the plain Mlp)",
                  batchnorm);
    return ht_init(h, "relax_head_train_init_ex", input_features, hidden_features, max_batch, batchnorm != 0);
}

int relax_head_train_arch(relax_handle* h, int* batchnorm) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, h->head_train.ready, "relax_head_train_arch: call relax_head_train_init first");
    RELAX_REQUIRE(h, batchnorm, "relax_head_train_arch: bad arguments");
    *batchnorm = h->head_train.batchnorm ? 1 : 0;
    return RELAX_OK;
}

int relax_head_train_import(relax_handle* h, int set, const float* const* tensors, const char* const* names, const int64_t* numels, int n,
                            int64_t num_batches_tracked, int64_t n_averaged) {
    if (!h) return RELAX_ERR_INVALID;
    HeadTrain& t = h->head_train;
    RELAX_REQUIRE(h, t.ready, "relax_head_train_import: call relax_head_train_init first");
    RELAX_REQUIRE(h, set >= 0 && set < HeadTrain::kSets && tensors && names && numels && n > 0, "relax_head_train_import: bad arguments");
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    if (!t.batchnorm) {
        RELAX_TRY(ht_refuse_bn_keys(h, "relax_head_train_import", names, n));
        RELAX_REQUIRE(h, num_batches_tracked == 0, "relax_head_train_import: num_batches_tracked %lld into a state without BatchNorm",
                      (long long)num_batches_tracked);
    }
    host::StateDict sd;
    for (int i = 0; i < n; ++i) {
        if (names[i] && std::string(names[i]) == "n_averaged") continue;
        sd.add(names[i], tensors[i], numels[i], /*strip_module=*/true);
    }
    const HtLayout L = ht_layout(t.Fpad, t.H1, t.H2, t.batchnorm);
    std::vector<HtItem> items = {{"fc1.bias", L.b1, t.H1}};
    if (t.batchnorm) {
        items.insert(items.end(), {{"bn1.weight", L.gamma, t.H1}, {"bn1.bias", L.beta, t.H1}, {"bn1.running_mean", L.rmean, t.H1},
                                   {"bn1.running_var", L.rvar, t.H1}});
    }
    items.insert(items.end(), {{"fc2.weight", L.w2, (int64_t)t.H2 * t.H1}, {"fc2.bias", L.b2, t.H2}, {"fc3.weight", L.w3, t.H2},
                               {"fc3.bias", L.b3, 1}});
    std::string err;
    const float* w1 = sd.get("fc1.weight", (int64_t)t.H1 * t.F, err, "mlp head state dict");
    RELAX_REQUIRE(h, w1, "%s", err.c_str());
    for (const HtItem& it : items) {
        const float* p = sd.get(it.key, it.numel, err, "mlp head state dict");
        RELAX_REQUIRE(h, p, "%s", err.c_str());
    }
    RELAX_HIP_CHECK(h, hipDeviceSynchronize());
    float* dst = t.set[set];
    RELAX_HIP_CHECK(h, hipMemset(dst, 0, sizeof(float) * L.n_all));
    RELAX_HIP_CHECK(h, hipMemcpy2D(dst + L.w1, sizeof(float) * t.Fpad, w1, sizeof(float) * t.F, sizeof(float) * t.F, t.H1,
                                   hipMemcpyHostToDevice));
    for (const HtItem& it : items) {
        const float* p = sd.get(it.key, it.numel, err, "mlp head state dict");
        RELAX_HIP_CHECK(h, hipMemcpy(dst + it.off, p, sizeof(float) * it.numel, hipMemcpyHostToDevice));
    }
    const int64_t c[2] = {num_batches_tracked, n_averaged};
    RELAX_HIP_CHECK(h, hipMemcpy(t.counters + 2 * set, c, sizeof(c), hipMemcpyHostToDevice));
    if (set == 0) {   // a fresh optimizer
        RELAX_HIP_CHECK(h, hipMemset(t.mom, 0, sizeof(float) * L.n_params));
        RELAX_HIP_CHECK(h, hipMemset(t.var, 0, sizeof(float) * L.n_params));
        t.adam_t = 0;
    }
    RELAX_HIP_CHECK(h, hipDeviceSynchronize());   // copies and fills are complete before the caller enqueues on its own stream
    return RELAX_OK;
}

int64_t relax_head_train_export_numel(relax_handle* h) {
    if (!h || !h->head_train.ready) return -1;
    const HeadTrain& t = h->head_train;
    return (int64_t)t.H1 * t.F + (t.batchnorm ? 5 : 1) * (int64_t)t.H1 + (int64_t)t.H2 * t.H1 + 2 * (int64_t)t.H2 + 1;
}

int relax_head_train_export(relax_handle* h, int set, int momentum, float* out, int64_t* counters, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    HeadTrain& t = h->head_train;
    RELAX_REQUIRE(h, t.ready, "relax_head_train_export: call relax_head_train_init first");
    RELAX_REQUIRE(h, set >= 0 && set < HeadTrain::kSets && out && counters, "relax_head_train_export: bad arguments");
    RELAX_REQUIRE(h, !momentum || set == 0, "relax_head_train_export: only the live set has momentum buffers");
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    RELAX_HIP_CHECK(h, hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    RELAX_TRY(ht_export_block(h, momentum ? t.mom : t.set[set], momentum != 0, out));
    RELAX_HIP_CHECK(h, hipMemcpy(counters, t.counters + 2 * set, sizeof(int64_t) * 2, hipMemcpyDeviceToHost));
    return RELAX_OK;
}

int relax_head_train_export_optimizer(relax_handle* h, int which, float* out, int64_t* t_out, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    HeadTrain& t = h->head_train;
    RELAX_REQUIRE(h, t.ready, "relax_head_train_export_optimizer: call relax_head_train_init first");
    RELAX_REQUIRE(h, (which == 0 || which == 1) && out && t_out, "relax_head_train_export_optimizer: bad arguments");
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    RELAX_HIP_CHECK(h, hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    RELAX_TRY(ht_export_block(h, which ? t.var : t.mom, true, out));
    *t_out = t.adam_t;
    return RELAX_OK;
}

int relax_head_train_import_optimizer(relax_handle* h, const float* const* exp_avg, const float* const* exp_avg_sq, const char* const* names,
                                      const int64_t* numels, int n, int64_t t_in) {
    if (!h) return RELAX_ERR_INVALID;
    HeadTrain& t = h->head_train;
    RELAX_REQUIRE(h, t.ready, "relax_head_train_import_optimizer: call relax_head_train_init first");
    RELAX_REQUIRE(h, exp_avg && exp_avg_sq && names && numels && n > 0 && t_in >= 0, "relax_head_train_import_optimizer: bad arguments");
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    if (!t.batchnorm) RELAX_TRY(ht_refuse_bn_keys(h, "relax_head_train_import_optimizer", names, n));
    const HtLayout L = ht_layout(t.Fpad, t.H1, t.H2, t.batchnorm);
    std::vector<HtItem> items = {{"fc1.bias", L.b1, t.H1}};
    if (t.batchnorm) items.insert(items.end(), {{"bn1.weight", L.gamma, t.H1}, {"bn1.bias", L.beta, t.H1}});
    items.insert(items.end(), {{"fc2.weight", L.w2, (int64_t)t.H2 * t.H1}, {"fc2.bias", L.b2, t.H2}, {"fc3.weight", L.w3, t.H2},
                               {"fc3.bias", L.b3, 1}});
    host::StateDict sd[2];
    for (int i = 0; i < n; ++i) {
        sd[0].add(names[i], exp_avg[i], numels[i], /*strip_module=*/true);
        sd[1].add(names[i], exp_avg_sq[i], numels[i], /*strip_module=*/true);
    }
    const char* what[2] = {"optimizer state exp_avg", "optimizer state exp_avg_sq"};
    std::string err;
    for (int k = 0; k < 2; ++k) {   // every tensor is there with its size before anything is written
        RELAX_REQUIRE(h, sd[k].get("fc1.weight", (int64_t)t.H1 * t.F, err, what[k]), "%s", err.c_str());
        for (const HtItem& it : items) RELAX_REQUIRE(h, sd[k].get(it.key, it.numel, err, what[k]), "%s", err.c_str());
    }
    RELAX_HIP_CHECK(h, hipDeviceSynchronize());
    float* dst[2] = {t.mom, t.var};
    for (int k = 0; k < 2; ++k) {
        RELAX_HIP_CHECK(h, hipMemset(dst[k], 0, sizeof(float) * L.n_params));
        RELAX_HIP_CHECK(h, hipMemcpy2D(dst[k] + L.w1, sizeof(float) * t.Fpad, sd[k].get("fc1.weight", -1, err, what[k]), sizeof(float) * t.F,
                                       sizeof(float) * t.F, t.H1, hipMemcpyHostToDevice));
        for (const HtItem& it : items)
            RELAX_HIP_CHECK(h, hipMemcpy(dst[k] + it.off, sd[k].get(it.key, it.numel, err, what[k]), sizeof(float) * it.numel, hipMemcpyHostToDevice));
    }
    t.adam_t = t_in;
    RELAX_HIP_CHECK(h, hipDeviceSynchronize());   // copies and fills are complete before the caller enqueues on its own stream
    return RELAX_OK;
}

int relax_head_train_copy(relax_handle* h, int dst_set, int src_set, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    HeadTrain& t = h->head_train;
    RELAX_REQUIRE(h, t.ready, "relax_head_train_copy: call relax_head_train_init first");
    RELAX_REQUIRE(h, dst_set >= 0 && dst_set < HeadTrain::kSets && src_set >= 0 && src_set < HeadTrain::kSets && dst_set != src_set,
                  "relax_head_train_copy: bad sets %d <- %d", dst_set, src_set);
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    RELAX_HIP_CHECK(h, hipMemcpyAsync(t.set[dst_set], t.set[src_set], sizeof(float) * t.n_all, hipMemcpyDeviceToDevice, s));
    RELAX_HIP_CHECK(h, hipMemcpyAsync(t.counters + 2 * dst_set, t.counters + 2 * src_set, sizeof(int64_t) * 2, hipMemcpyDeviceToDevice, s));
    return RELAX_OK;
}

int relax_head_criterion(relax_handle* h, const float* pred, const float* target, int B, float l1_w, float rank_w, float* loss,
                         float* grad, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    HeadTrain& t = h->head_train;
    RELAX_REQUIRE(h, t.ready, "relax_head_criterion: call relax_head_train_init first");
    RELAX_REQUIRE(h, pred && target && loss && B >= 1 && B <= t.max_batch, "relax_head_criterion: bad arguments (B = %d, at most %d)", B,
                  t.max_batch);
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const HtAct A = ht_act(t.max_batch, t.H1, t.H2);
    hipLaunchKernelGGL(ht_criterion, dim3((unsigned)B), dim3(256), 0, s, pred, target, B, l1_w, rank_w, t.act + A.rowloss, grad);
    hipLaunchKernelGGL(ht_loss_finish, dim3(1), dim3(256), 0, s, t.act + A.rowloss, B, (double*)nullptr, loss);
    RELAX_HIP_CHECK(h, hipGetLastError());
    return RELAX_OK;
}

int relax_head_train_step(relax_handle* h, const float* xp, const float* target, int n, const int32_t* index, int B, float lr,
                          float momentum, float weight_decay, float l1_w, float rank_w, float drop_rate, uint64_t seed, uint64_t step,
                          uint8_t* mask1, uint8_t* mask2, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_TRY(ht_check_batch(h, "relax_head_train_step", xp, index, n, B, 2));
    RELAX_REQUIRE(h, target, "relax_head_train_step: no targets");
    RELAX_REQUIRE(h, drop_rate >= 0.f && drop_rate < 1.f, "relax_head_train_step: drop_rate %g outside [0, 1)", (double)drop_rate);
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    return ht_step(h, xp, target, n, index, B, HtSgd{lr, momentum, weight_decay}, l1_w, rank_w, drop_rate, seed, step,
                   mask1, mask2, static_cast<hipStream_t>(stream));
}

int relax_head_train_step_adam(relax_handle* h, const float* xp, const float* target, int n, const int32_t* index, int B, double lr,
                               double beta1, double beta2, double eps, double weight_decay, int decoupled, float l1_w, float rank_w,
                               float drop_rate, uint64_t seed, uint64_t step, uint8_t* mask1, uint8_t* mask2, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_TRY(ht_check_batch(h, "relax_head_train_step_adam", xp, index, n, B, 2));
    RELAX_REQUIRE(h, target, "relax_head_train_step_adam: no targets");
    RELAX_REQUIRE(h, drop_rate >= 0.f && drop_rate < 1.f, "relax_head_train_step_adam: drop_rate %g outside [0, 1)", (double)drop_rate);
    RELAX_REQUIRE(h, beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0,
                  "relax_head_train_step_adam: betas (%g, %g) outside [0, 1) or eps %g below 0", beta1, beta2, eps);
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    HeadTrain& t = h->head_train;
    const HtAdam adam = make_adam(lr, beta1, beta2, eps, weight_decay, decoupled, t.adam_t + 1);
    RELAX_TRY(ht_step(h, xp, target, n, index, B, adam, l1_w, rank_w, drop_rate, seed, step, mask1, mask2,
                      static_cast<hipStream_t>(stream)));
    t.adam_t += 1;
    return RELAX_OK;
}

int relax_head_train_eval(relax_handle* h, int set, const float* xp, const float* target, int n, const int32_t* index, int B, float l1_w,
                          float rank_w, float* pred, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_TRY(ht_check_batch(h, "relax_head_train_eval", xp, index, n, B, 1));
    RELAX_REQUIRE(h, set >= 0 && set < HeadTrain::kSets && pred, "relax_head_train_eval: bad arguments");
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HeadTrain& t = h->head_train;
    const int H1 = t.H1, H2 = t.H2, Fpad = t.Fpad;
    const HtLayout L = ht_layout(Fpad, H1, H2, t.batchnorm);
    const HtAct A = ht_act(t.max_batch, H1, H2);
    const float* P = t.set[set];
    float* a = t.act;
    const int64_t n1 = (int64_t)B * H1;
    hipLaunchKernelGGL(ht_gather, gather_grid(B, Fpad), dim3(256), 0, s, xp, target, index, n, Fpad, t.xb, a + A.yb, (int64_t*)nullptr);
    if (t.batchnorm) {
        RELAX_TRY(ht_gemm(h, t.xb, P + L.w1, P + L.b1, a + A.z1, B, H1, Fpad, 0, s));
        hipLaunchKernelGGL(ht_bn_eval, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, s, a + A.z1, n1, H1, P + L.gamma, P + L.beta, P + L.rmean,
                           P + L.rvar, a + A.a1);
    } else {   // a1 = GELU(z1): the contraction's own epilogue, as fc2 below
        RELAX_TRY(ht_gemm(h, t.xb, P + L.w1, P + L.b1, a + A.a1, B, H1, Fpad, 2, s));
    }
    RELAX_TRY(ht_gemm(h, a + A.a1, P + L.w2, P + L.b2, a + A.z2, B, H2, H1, 2, s));
    hipLaunchKernelGGL(ht_fwd_tail, dim3((unsigned)B), dim3(256), 0, s, a + A.z2, H2, P + L.w3, P + L.b3, 0, a + A.a2, pred, HtDrop{},
                       (uint8_t*)nullptr);
    if (target) {
        hipLaunchKernelGGL(ht_criterion, dim3((unsigned)B), dim3(256), 0, s, pred, a + A.yb, B, l1_w, rank_w, a + A.rowloss, (float*)nullptr);
        hipLaunchKernelGGL(ht_loss_finish, dim3(1), dim3(256), 0, s, a + A.rowloss, B, t.loss + 3, (float*)nullptr);
    }
    RELAX_HIP_CHECK(h, hipGetLastError());
    return RELAX_OK;
}

int relax_head_train_bn_pass(relax_handle* h, int set, int reset, const float* xp, int n, const int32_t* index, int B, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    HeadTrain& t = h->head_train;
    RELAX_REQUIRE(h, t.ready, "relax_head_train_bn_pass: call relax_head_train_init first");
    RELAX_REQUIRE(h, set >= 0 && set < HeadTrain::kSets, "relax_head_train_bn_pass: bad set %d", set);
    if (!t.batchnorm) {   // no BatchNorm to refresh (update_bn returns at once for such a model): the arguments are checked, nothing is launched
        if (B > 0) RELAX_TRY(ht_check_batch(h, "relax_head_train_bn_pass", xp, index, n, B, 2));
        return RELAX_OK;
    }
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int H1 = t.H1, H2 = t.H2, Fpad = t.Fpad;
    const HtLayout L = ht_layout(Fpad, H1, H2, t.batchnorm);
    const HtAct A = ht_act(t.max_batch, H1, H2);
    float* P = t.set[set];
    int64_t* nbt = t.counters + 2 * set;
    if (reset) hipLaunchKernelGGL(ht_bn_reset, dim3((unsigned)((H1 + 255) / 256)), dim3(256), 0, s, P + L.rmean, P + L.rvar, H1, nbt);
    if (B > 0) {
        RELAX_TRY(ht_check_batch(h, "relax_head_train_bn_pass", xp, index, n, B, 2));
        float* a = t.act;
        hipLaunchKernelGGL(ht_gather, gather_grid(B, Fpad), dim3(256), 0, s, xp, (const float*)nullptr, index, n, Fpad, t.xb, a + A.yb, nbt);
        RELAX_TRY(ht_gemm(h, t.xb, P + L.w1, P + L.b1, a + A.z1, B, H1, Fpad, 0, s));
        hipLaunchKernelGGL(ht_bn_fwd, dim3((unsigned)H1), dim3(256), 0, s, a + A.z1, B, H1, P + L.gamma, P + L.beta, P + L.rmean, P + L.rvar, nbt,
                           1, (float*)nullptr, (float*)nullptr, (float*)nullptr, HtDrop{}, (uint8_t*)nullptr);
    }
    RELAX_HIP_CHECK(h, hipGetLastError());
    return RELAX_OK;
}

int relax_head_train_swa_update(relax_handle* h, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    HeadTrain& t = h->head_train;
    RELAX_REQUIRE(h, t.ready, "relax_head_train_swa_update: call relax_head_train_init first");
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t total = (int64_t)t.n_params;
    hipLaunchKernelGGL(ht_swa_update, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, t.set[0], t.set[1], total, t.counters + 3);
    hipLaunchKernelGGL(ht_count, dim3(1), dim3(1), 0, s, t.counters + 3, (int64_t)1);
    RELAX_HIP_CHECK(h, hipGetLastError());
    return RELAX_OK;
}

static int ht_pad_abs_sum(relax_handle* h, const char* what, int blocks, double* out, relax_stream stream) {
    HeadTrain& t = h->head_train;
    RELAX_REQUIRE(h, t.ready && out, "%s: no state, or bad arguments", what);
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    RELAX_HIP_CHECK(h, hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    for (int k = 0; k < blocks; ++k) out[k] = 0.0;
    const int pad = t.Fpad - t.F;
    if (pad == 0) return RELAX_OK;
    std::vector<float> host((size_t)t.H1 * pad);
    const float* src[3] = {t.set[0], t.mom, t.var};
    for (int k = 0; k < blocks; ++k) {
        RELAX_HIP_CHECK(h, hipMemcpy2D(host.data(), sizeof(float) * pad, src[k] + t.F, sizeof(float) * t.Fpad, sizeof(float) * pad, t.H1,
                                       hipMemcpyDeviceToHost));
        for (float v : host) out[k] += std::fabs((double)v);
    }
    return RELAX_OK;
}

int relax_head_train_pad_abs_sum(relax_handle* h, double* out, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    return ht_pad_abs_sum(h, "relax_head_train_pad_abs_sum", 2, out, stream);
}

int relax_head_train_pad_abs_sum_adam(relax_handle* h, double* out, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    return ht_pad_abs_sum(h, "relax_head_train_pad_abs_sum_adam", 3, out, stream);
}

static int ht_grad_w1(relax_handle* h) {   // only the unfused measurements ever materialise the gradient of fc1.weight
    HeadTrain& t = h->head_train;
    if (t.grad_w1) return RELAX_OK;
    t.grad_w1 = static_cast<float*>(t.mem.keep(h, sizeof(float) * (size_t)t.H1 * t.Fpad, "the unfused fc1.weight gradient"));
    return t.grad_w1 ? RELAX_OK : RELAX_ERR_NOMEM;
}

int relax_head_train_dw1(relax_handle* h, int fused, int B, float lr, float momentum, float weight_decay, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    HeadTrain& t = h->head_train;
    RELAX_REQUIRE(h, t.ready, "relax_head_train_dw1: call relax_head_train_init first");
    RELAX_REQUIRE(h, B >= 2 && B <= t.max_batch, "relax_head_train_dw1: batch of %d rows (this state takes 2..%d)", B, t.max_batch);
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const HtLayout L = ht_layout(t.Fpad, t.H1, t.H2, t.batchnorm);
    const HtAct A = ht_act(t.max_batch, t.H1, t.H2);
    const HtSgd sgd{lr, momentum, weight_decay};
    const dim3 grid((unsigned)(t.H1 / kDwTJ), (unsigned)((t.Fpad + kDwTF - 1) / kDwTF));
    if (fused) {
        hipLaunchKernelGGL(ht_dw1_sgd<true>, grid, dim3(256), 0, s, t.act + A.dz1, t.xb, B, t.H1, t.Fpad, t.set[0] + L.w1, t.mom + L.w1, sgd,
                           (float*)nullptr);
    } else {
        const size_t nw1 = (size_t)t.H1 * t.Fpad;
        RELAX_TRY(ht_grad_w1(h));
        hipLaunchKernelGGL(ht_dw1_sgd<false>, grid, dim3(256), 0, s, t.act + A.dz1, t.xb, B, t.H1, t.Fpad, t.set[0] + L.w1, t.mom + L.w1, sgd,
                           t.grad_w1);
        const int64_t n4 = (int64_t)(nw1 / 4);
        hipLaunchKernelGGL(ht_sgd_apply, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, t.grad_w1, t.set[0] + L.w1, t.mom + L.w1, n4, sgd);
    }
    RELAX_HIP_CHECK(h, hipGetLastError());
    return RELAX_OK;
}

int relax_head_train_dw1_adam(relax_handle* h, int fused, int B, double lr, double beta1, double beta2, double eps, double weight_decay,
                              int decoupled, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    HeadTrain& t = h->head_train;
    RELAX_REQUIRE(h, t.ready, "relax_head_train_dw1_adam: call relax_head_train_init first");
    RELAX_REQUIRE(h, B >= 2 && B <= t.max_batch, "relax_head_train_dw1_adam: batch of %d rows (this state takes 2..%d)", B, t.max_batch);
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const HtAct A = ht_act(t.max_batch, t.H1, t.H2);
    const HtAdam adam = make_adam(lr, beta1, beta2, eps, weight_decay, decoupled, std::max<int64_t>(t.adam_t, 1));   // the step count stays
    if (fused) {
        launch_dw1(t, t.act + A.dz1, B, t.set[0], adam, s);
    } else {
        RELAX_TRY(ht_grad_w1(h));
        hipLaunchKernelGGL(ht_dw1_adam<false>, dim3((unsigned)(t.H1 / kDwTJ), (unsigned)((t.Fpad + kDwTF - 1) / kDwTF)), dim3(256), 0, s,
                           t.act + A.dz1, t.xb, B, t.H1, t.Fpad, t.set[0], t.mom, t.var, adam, t.grad_w1);
        const int64_t n4 = (int64_t)t.H1 * t.Fpad / 4;
        hipLaunchKernelGGL(ht_adam_apply, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, t.grad_w1, t.set[0], t.mom, t.var, n4, adam);
    }
    RELAX_HIP_CHECK(h, hipGetLastError());
    return RELAX_OK;
}

int relax_head_train_loss_read(relax_handle* h, int which, int reset, double* out, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    HeadTrain& t = h->head_train;
    RELAX_REQUIRE(h, t.ready, "relax_head_train_loss_read: call relax_head_train_init first");
    RELAX_REQUIRE(h, (which == 0 || which == 1) && out, "relax_head_train_loss_read: bad arguments");
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    RELAX_HIP_CHECK(h, hipMemcpyAsync(out, t.loss + 3 * which, sizeof(double) * 3, hipMemcpyDeviceToHost, s));
    if (reset) RELAX_HIP_CHECK(h, fill_async(t.loss + 3 * which, 0, sizeof(double) * 3, s));
    RELAX_HIP_CHECK(h, hipStreamSynchronize(s));
    return RELAX_OK;
}

}  // extern "C"
