// The metrics core of metrics_core.h as plain host C++ (one thread, sums in order): the yardstick of the device kernels
// (make metrics_host) and, built alone under AddressSanitizer + UBSan (make sanitize_metrics), the subject of
// tests/test_metrics_sanitized.py.  Driven by tests/metrics_driver.py.  Not part of librelax_hip.so.
#include <vector>

#include "metrics_core.h"

// flags: 1 = rank statistics (out_k[8], counts [5][n] if not null), 2 = logistic fit (out[17], fitted [n] if not null).
// p0: the start of the fit, or null for the reference's [max(y_true), min(y_true), mean(y_pred), 0.5].
// Returns 0, or 1 for bad arguments.
extern "C" int relax_metrics_host(const double* y_true, const double* y_pred, int n, int flags, const double* p0, double* out_k,
                                  int32_t* counts, double* out, double* fitted) {
    if (!y_true || !y_pred || n < mtr::kMinN || n > mtr::kMaxN) return 1;
    if (((flags & 1) && !out_k) || ((flags & 2) && !out)) return 1;
    int64_t nonfinite = 0;
    for (int i = 0; i < n; ++i) nonfinite += (mtr::is_finite(y_true[i]) && mtr::is_finite(y_pred[i])) ? 0 : 1;
    if (flags & 1) {
        mtr::RankSums r = {0, 0, 0, 0, 0, 0, 0};
        for (int i = 0; i < n; ++i) {
            mtr::PairCount c = {0, 0, 0, 0, 0};
            for (int j = 0; j < n; ++j) mtr::pair_update(c, y_true[i], y_pred[i], y_true[j], y_pred[j]);
            mtr::rank_accumulate(r, c, n, mtr::is_finite(y_true[i]) && mtr::is_finite(y_pred[i]));
            if (counts) {
                const size_t N = (size_t)n;
                counts[i] = (int32_t)c.less_x;
                counts[N + i] = (int32_t)c.equal_x;
                counts[2 * N + i] = (int32_t)c.less_y;
                counts[3 * N + i] = (int32_t)c.equal_y;
                counts[4 * N + i] = c.s;
            }
        }
        mtr::rank_finish(r, n, out_k);
    }
    if (!(flags & 2)) return 0;
    if (nonfinite) {
        for (int k = 0; k < mtr::O_COUNT; ++k) out[k] = mtr::quiet_nan();
        out[mtr::O_ITER] = out[mtr::O_CONVERGED] = 0.0;
        out[mtr::O_NONFINITE] = (double)nonfinite;
        if (fitted)
            for (int i = 0; i < n; ++i) fitted[i] = mtr::quiet_nan();
        return 0;
    }
    double start[4];
    if (p0) {
        for (int i = 0; i < 4; ++i) start[i] = p0[i];
    } else {
        double mx = y_true[0], mn = y_true[0], sx = 0;
        for (int i = 0; i < n; ++i) {
            mx = y_true[i] > mx ? y_true[i] : mx;
            mn = y_true[i] < mn ? y_true[i] : mn;
            sx += y_pred[i];
        }
        start[0] = mx, start[1] = mn, start[2] = sx / (double)n, start[3] = 0.5;
    }
    mtr::Lm lm;
    mtr::lm_begin(lm, start);
    for (;;) {
        mtr::Sums s;
        mtr::sums_zero(s);
        for (int i = 0; i < n; ++i) mtr::sums_row(s, lm.trial, y_pred[i], y_true[i]);
        if (!mtr::lm_advance(lm, s)) break;
    }
    std::vector<double> f((size_t)n);
    double sy = 0, sf = 0;
    for (int i = 0; i < n; ++i) {
        f[i] = mtr::model(lm.p, y_pred[i]);
        sy += y_true[i];
        sf += f[i];
    }
    const double my = sy / (double)n, mf = sf / (double)n;
    double syy = 0, sff = 0, syf = 0, sse = 0;
    for (int i = 0; i < n; ++i) {
        syy += (y_true[i] - my) * (y_true[i] - my);
        sff += (f[i] - mf) * (f[i] - mf);
        syf += (y_true[i] - my) * (f[i] - mf);
        sse += (f[i] - y_true[i]) * (f[i] - y_true[i]);
    }
    mtr::lm_report(lm, out);
    out[mtr::O_PLCC] = mtr::pearson_from_centred(syy, sff, syf);
    out[mtr::O_RMSE] = sqrt(sse / (double)n);
    out[mtr::O_SRCC] = (flags & 1) ? out_k[mtr::K_SRCC] : mtr::quiet_nan();
    out[mtr::O_KRCC] = (flags & 1) ? out_k[mtr::K_KRCC] : mtr::quiet_nan();
    out[mtr::O_NONFINITE] = 0.0;
    if (fitted)
        for (int i = 0; i < n; ++i) fitted[i] = f[i];
    return 0;
}
