// Correlation metrics of a head's predictions on gfx950 (include/relax_hip.h: relax_metrics_*): the pair pass behind Kendall's
// tau-b and Spearman's rho, and the Levenberg-Marquardt fit of the 4-parameter logistic behind PLCC and RMSE.
//   mt_pair       the n x n comparison in tiles: a thread owns one element i, a workgroup stages kTile elements j in LDS and
//                 every lane reads the same j (an LDS broadcast); five 32-bit counters per element, added with integer atomics
//                 when several column tiles meet on a row - integer sums, so the result does not depend on the order
//   mt_rank       one workgroup: 64-bit sums of the counters -> S, n1, n2, the centred rank sums -> krcc, srcc
//   mt_fit        one persistent workgroup: p0, then the LM loop of metrics_core.h with no host round trip - the 15 sums of an
//                 iteration go through a fixed tree (64 lanes by shuffles, 16 waves in order), lane 0 takes the 4x4 step
// The arithmetic that decides a result is metrics_core.h's, shared with the host build (metrics_host.cpp).
#include "metrics_core.h"
#include "relax_internal.h"

namespace relax {
namespace {

constexpr int kPairThreads = 256;
constexpr int kTile = 1024;          // elements j per workgroup: 16 KiB of LDS
constexpr int kFitThreads = 1024;
constexpr int kWaves = kFitThreads / 64;

__global__ __launch_bounds__(kPairThreads) void mt_pair(const double* __restrict__ x, const double* __restrict__ y, int n,
                                                        uint32_t* __restrict__ counts) {
    __shared__ double2 tile[kTile];
    const int col0 = blockIdx.y * kTile;
    const int cols = min(kTile, n - col0);
    for (int t = threadIdx.x; t < cols; t += kPairThreads) tile[t] = make_double2(x[col0 + t], y[col0 + t]);
    __syncthreads();
    const int i = blockIdx.x * kPairThreads + threadIdx.x;
    if (i >= n) return;
    const double xi = x[i], yi = y[i];
    mtr::PairCount c = {0, 0, 0, 0, 0};
#pragma unroll 4
    for (int t = 0; t < cols; ++t) {
        const double2 v = tile[t];
        mtr::pair_update(c, xi, yi, v.x, v.y);
    }
    const size_t N = (size_t)n;
    atomicAdd(counts + i, c.less_x);
    atomicAdd(counts + N + i, c.equal_x);
    atomicAdd(counts + 2 * N + i, c.less_y);
    atomicAdd(counts + 3 * N + i, c.equal_y);
    atomicAdd(reinterpret_cast<int*>(counts + 4 * N) + i, c.s);
}

// ---- fixed-tree reductions of one workgroup of kFitThreads ----------------------------------------------------------------
struct OpAdd { template <class T> __device__ static T f(T a, T b) { return a + b; } };
struct OpMax { template <class T> __device__ static T f(T a, T b) { return a > b ? a : b; } };
struct OpMin { template <class T> __device__ static T f(T a, T b) { return a < b ? a : b; } };

template <class Op>
__device__ inline double wave_reduce(double v) {
    for (int off = 32; off > 0; off >>= 1) v = Op::f(v, __shfl_down(v, off, 64));
    return v;
}
__device__ inline long long wave_reduce_i64(long long v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// every lane gets the result; `part` holds kWaves + 1 doubles
template <class Op>
__device__ inline double block_reduce(double v, double* part) {
    v = wave_reduce<Op>(v);
    __syncthreads();   // the previous use of `part` is over
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = part[0];
        for (int w = 1; w < kWaves; ++w) t = Op::f(t, part[w]);
        part[kWaves] = t;
    }
    __syncthreads();
    return part[kWaves];
}

__global__ __launch_bounds__(kFitThreads) void mt_rank(const double* __restrict__ x, const double* __restrict__ y,
                                                       const uint32_t* __restrict__ counts, int n, double* __restrict__ out) {
    __shared__ long long part[kWaves][7];
    mtr::RankSums r = {0, 0, 0, 0, 0, 0, 0};
    const size_t N = (size_t)n;
    for (int i = threadIdx.x; i < n; i += kFitThreads) {
        mtr::PairCount c;
        c.less_x = counts[i];
        c.equal_x = counts[N + i];
        c.less_y = counts[2 * N + i];
        c.equal_y = counts[3 * N + i];
        c.s = (int32_t)counts[4 * N + i];
        mtr::rank_accumulate(r, c, n, mtr::is_finite(x[i]) && mtr::is_finite(y[i]));
    }
    long long v[7] = {r.s2, r.tx, r.ty, r.dxy, r.dxx, r.dyy, r.nonfinite};
    for (int k = 0; k < 7; ++k) {
        const long long t = wave_reduce_i64(v[k]);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][k] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long t[7];
        for (int k = 0; k < 7; ++k) {
            t[k] = 0;
            for (int w = 0; w < kWaves; ++w) t[k] += part[w][k];
        }
        const mtr::RankSums tot = {t[0], t[1], t[2], t[3], t[4], t[5], t[6]};
        mtr::rank_finish(tot, n, out);
    }
}

__global__ __launch_bounds__(kFitThreads) void mt_fit(const double* __restrict__ y_true, const double* __restrict__ y_pred, int n,
                                                      const double* __restrict__ rank_out, double* __restrict__ out,
                                                      double* __restrict__ fitted) {
    __shared__ double part[kWaves + 1];
    __shared__ double wsum[kWaves][mtr::kSums];
    __shared__ mtr::Lm lm;
    __shared__ mtr::Sums total;
    __shared__ int more;
    const int tid = threadIdx.x;

    // p0 = [max(y_true), min(y_true), mean(y_pred), 0.5] and the count of non-finite inputs
    double mx = -INFINITY, mn = INFINITY, sx = 0, bad = 0;
    for (int i = tid; i < n; i += kFitThreads) {
        const double yt = y_true[i], yp = y_pred[i];
        mx = yt > mx ? yt : mx;
        mn = yt < mn ? yt : mn;
        sx += yp;
        bad += (mtr::is_finite(yt) && mtr::is_finite(yp)) ? 0.0 : 1.0;
    }
    mx = block_reduce<OpMax>(mx, part);
    mn = block_reduce<OpMin>(mn, part);
    sx = block_reduce<OpAdd>(sx, part);
    bad = block_reduce<OpAdd>(bad, part);
    if (bad != 0.0) {   // not an error: every metric is nan and the count says why
        if (tid == 0) {
            for (int k = 0; k < mtr::O_COUNT; ++k) out[k] = mtr::quiet_nan();
            out[mtr::O_ITER] = 0.0;
            out[mtr::O_CONVERGED] = 0.0;
            out[mtr::O_NONFINITE] = bad;
        }
        if (fitted)
            for (int i = tid; i < n; i += kFitThreads) fitted[i] = mtr::quiet_nan();
        return;
    }
    if (tid == 0) {
        const double p0[4] = {mx, mn, sx / (double)n, 0.5};
        mtr::lm_begin(lm, p0);
    }
    __syncthreads();

    for (;;) {
        const double p[4] = {lm.trial[0], lm.trial[1], lm.trial[2], lm.trial[3]};
        mtr::Sums s;
        mtr::sums_zero(s);
        for (int i = tid; i < n; i += kFitThreads) mtr::sums_row(s, p, y_pred[i], y_true[i]);
        double v[mtr::kSums];
        for (int k = 0; k < 10; ++k) v[k] = s.a[k];
        for (int k = 0; k < 4; ++k) v[10 + k] = s.g[k];
        v[14] = s.c;
        for (int k = 0; k < mtr::kSums; ++k) {
            const double t = wave_reduce<OpAdd>(v[k]);
            if ((tid & 63) == 0) wsum[tid >> 6][k] = t;
        }
        __syncthreads();
        if (tid < mtr::kSums) {
            double t = wsum[0][tid];
            for (int w = 1; w < kWaves; ++w) t += wsum[w][tid];
            if (tid < 10) total.a[tid] = t;
            else if (tid < 14) total.g[tid - 10] = t;
            else total.c = t;
        }
        __syncthreads();
        if (tid == 0) more = mtr::lm_advance(lm, total) ? 1 : 0;
        __syncthreads();
        if (!more) break;
    }

    // the fitted scores, rmse and plcc = pearson(y_true, fitted) from centred sums
    const double p[4] = {lm.p[0], lm.p[1], lm.p[2], lm.p[3]};
    double sy = 0, sf = 0;
    for (int i = tid; i < n; i += kFitThreads) {
        const double f = mtr::model(p, y_pred[i]);
        if (fitted) fitted[i] = f;
        sy += y_true[i];
        sf += f;
    }
    const double my = block_reduce<OpAdd>(sy, part) / (double)n;
    const double mf = block_reduce<OpAdd>(sf, part) / (double)n;
    double syy = 0, sff = 0, syf = 0, sse = 0;
    for (int i = tid; i < n; i += kFitThreads) {
        const double yt = y_true[i], f = mtr::model(p, y_pred[i]);
        syy += (yt - my) * (yt - my);
        sff += (f - mf) * (f - mf);
        syf += (yt - my) * (f - mf);
        sse += (f - yt) * (f - yt);
    }
    syy = block_reduce<OpAdd>(syy, part);
    sff = block_reduce<OpAdd>(sff, part);
    syf = block_reduce<OpAdd>(syf, part);
    sse = block_reduce<OpAdd>(sse, part);
    if (tid == 0) {
        mtr::lm_report(lm, out);
        out[mtr::O_PLCC] = mtr::pearson_from_centred(syy, sff, syf);
        out[mtr::O_RMSE] = sqrt(sse / (double)n);
        out[mtr::O_SRCC] = rank_out[mtr::K_SRCC];
        out[mtr::O_KRCC] = rank_out[mtr::K_KRCC];
        out[mtr::O_NONFINITE] = 0.0;
    }
}

// workspace of one call: counters [5][n] uint32 | rank_out [8] | out [O_COUNT] (doubles, 8-byte aligned)
struct Ws {
    uint32_t* counts;
    double* rank_out;
    double* out;
};

size_t counts_bytes(int n) { return ((size_t)5 * n * sizeof(uint32_t) + 7) / 8 * 8; }

int metrics_ws(relax_handle* h, int n, Ws* ws) {
    size_t cap = 4096;
    while (cap < (size_t)n) cap *= 2;   // grows in powers of two: a run over folds of rising size reallocates a few times, not every call
    RELAX_TRY(ensure_buf(h, h->metrics_ws, counts_bytes((int)cap) + sizeof(double) * (mtr::K_COUNT + mtr::O_COUNT)));
    char* base = static_cast<char*>(h->metrics_ws.p);
    ws->counts = reinterpret_cast<uint32_t*>(base);
    ws->rank_out = reinterpret_cast<double*>(base + counts_bytes((int)cap));
    ws->out = ws->rank_out + mtr::K_COUNT;
    return RELAX_OK;
}

bool on_device(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();   // an ordinary host pointer is not an error of ours
        return false;
    }
    return a.type == hipMemoryTypeDevice;
}

int pair_pass(relax_handle* h, const double* x, const double* y, int n, const Ws& ws, hipStream_t s) {
    RELAX_HIP_CHECK(h, fill_async(ws.counts, 0, (size_t)5 * n * sizeof(uint32_t), s));
    const dim3 grid((unsigned)((n + kPairThreads - 1) / kPairThreads), (unsigned)((n + kTile - 1) / kTile));
    hipLaunchKernelGGL(mt_pair, grid, dim3(kPairThreads), 0, s, x, y, n, ws.counts);
    hipLaunchKernelGGL(mt_rank, dim3(1), dim3(kFitThreads), 0, s, x, y, ws.counts, n, ws.rank_out);
    RELAX_HIP_CHECK(h, hipGetLastError());
    return RELAX_OK;
}

// the results to the caller: a device `out` was written in place; a host `out` is copied and waited for
int deliver(relax_handle* h, const double* dev, double* out, int count, bool out_on_device, hipStream_t s) {
    if (out_on_device) return RELAX_OK;
    RELAX_HIP_CHECK(h, hipMemcpyAsync(out, dev, sizeof(double) * count, hipMemcpyDeviceToHost, s));
    RELAX_HIP_CHECK(h, hipStreamSynchronize(s));
    return RELAX_OK;
}

}  // namespace
}  // namespace relax

using namespace relax;

extern "C" {

int relax_metrics_kendall(relax_handle* h, const double* x, const double* y, int n, double* out, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, x && y && out, "relax_metrics_kendall: null pointer");
    RELAX_REQUIRE(h, n >= mtr::kMinN && n <= mtr::kMaxN, "relax_metrics_kendall: n = %d outside [%d, %d]", n, mtr::kMinN, mtr::kMaxN);
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    Ws ws;
    RELAX_TRY(metrics_ws(h, n, &ws));
    const bool dev_out = on_device(out);
    if (dev_out) ws.rank_out = out;
    RELAX_TRY(pair_pass(h, x, y, n, ws, s));
    return deliver(h, ws.rank_out, out, mtr::K_COUNT, dev_out, s);
}

int relax_metrics_pair_counts(relax_handle* h, const double* x, const double* y, int n, int32_t* counts, relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, x && y && counts, "relax_metrics_pair_counts: null pointer");
    RELAX_REQUIRE(h, n >= mtr::kMinN && n <= mtr::kMaxN, "relax_metrics_pair_counts: n = %d outside [%d, %d]", n, mtr::kMinN, mtr::kMaxN);
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    Ws ws;
    RELAX_TRY(metrics_ws(h, n, &ws));
    RELAX_TRY(pair_pass(h, x, y, n, ws, s));
    RELAX_HIP_CHECK(h, hipMemcpyAsync(counts, ws.counts, (size_t)5 * n * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    return RELAX_OK;
}

int relax_metrics_correlation(relax_handle* h, const double* y_true, const double* y_pred, int n, double* out, double* y_pred_logistic,
                              relax_stream stream) {
    if (!h) return RELAX_ERR_INVALID;
    RELAX_REQUIRE(h, y_true && y_pred && out, "relax_metrics_correlation: null pointer");
    RELAX_REQUIRE(h, n >= mtr::kMinN && n <= mtr::kMaxN, "relax_metrics_correlation: n = %d outside [%d, %d]", n, mtr::kMinN, mtr::kMaxN);
    RELAX_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    Ws ws;
    RELAX_TRY(metrics_ws(h, n, &ws));
    const bool dev_out = on_device(out);
    if (dev_out) ws.out = out;
    RELAX_TRY(pair_pass(h, y_true, y_pred, n, ws, s));
    hipLaunchKernelGGL(mt_fit, dim3(1), dim3(kFitThreads), 0, s, y_true, y_pred, n, ws.rank_out, ws.out, y_pred_logistic);
    RELAX_HIP_CHECK(h, hipGetLastError());
    return deliver(h, ws.out, out, mtr::O_COUNT, dev_out, s);
}

}  // extern "C"
