// Correlation metrics core: the rank statistics from integer pair counts (Kendall's tau-b, Spearman's rho) and the
// Levenberg-Marquardt fit of the 4-parameter logistic  f(x) = b2 + (b1 - b2) / (1 + exp(-(x - b3) / |b4|)).  One source, two builds:
//   - metrics.hip: the pair pass as a tiled n x n kernel, the fit as one persistent workgroup on gfx950;
//   - metrics_host.cpp: one thread of host code (tests/metrics_driver.py; also built alone under AddressSanitizer + UBSan).
// Everything that decides a result lives here: what one pair contributes, how the counts become krcc / srcc, the model and its
// Jacobian row, the damped 4x4 solve, the step-acceptance and the stopping rule.  The two builds differ in who sums the 15
// per-iteration sums over n (a fixed tree of 1024 lanes / one thread in order), nothing else.
// Values are fp64, counts are 64-bit integers; no fast-math, so sqrt and division round as IEEE-754 says on both sides.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MTR_HD __host__ __device__
#else
#define MTR_HD
#endif

namespace mtr {

constexpr int kMinN = 2;
constexpr int kMaxN = 131072;        // n^3 <= 2^51: the centred rank sums stay exact in int64 and in fp64
constexpr double kTol = 1.49e-8;     // ftol = xtol of MINPACK as scipy.optimize.curve_fit sets them (sqrt of the fp64 epsilon)
constexpr int kMaxIter = 400;        // trial points, accepted or not
constexpr double kLambda0 = 1e-3, kLambdaMin = 1e-12, kLambdaMax = 1e12;

// out[] of relax_metrics_correlation (include/relax_hip.h)
enum { O_PLCC = 0, O_RMSE, O_SRCC, O_KRCC, O_POPT, O_ITER = 8, O_CONVERGED, O_COST0, O_COST, O_NONFINITE, O_P0, O_COUNT = 17 };
// out[] of relax_metrics_kendall
enum { K_KRCC = 0, K_SRCC, K_S, K_N1, K_N2, K_N0, K_NONFINITE, K_COUNT = 8 };

// ---- rank statistics ---------------------------------------------------------------------------------------------------
// What element j adds to element i's counters: how many values lie below / equal (itself included) in each vector, and
// sign(xi - xj) * sign(yi - yj), whose sum over all ordered pairs is 2 S (the diagonal adds 0).
struct PairCount {
    uint32_t less_x, equal_x, less_y, equal_y;
    int32_t s;
};

MTR_HD inline void pair_update(PairCount& c, double xi, double yi, double xj, double yj) {
    const int lx = xj < xi, gx = xj > xi, ly = yj < yi, gy = yj > yi;
    c.less_x += (uint32_t)lx;
    c.equal_x += (uint32_t)(xj == xi);
    c.less_y += (uint32_t)ly;
    c.equal_y += (uint32_t)(yj == yi);
    c.s += (lx - gx) * (ly - gy);
}

// Sums over the elements of what the finish needs.  With r = less + (equal + 1) / 2 the average rank, d = 2 r - (n + 1) =
// 2 less + equal - n is an integer (the mean rank is (n + 1) / 2 whatever the ties), |d| < n.
struct RankSums {
    int64_t s2;            // sum of PairCount::s = 2 S
    int64_t tx, ty;        // sum of (equal - 1) = 2 n1, 2 n2
    int64_t dxy, dxx, dyy; // sums of dx dy, dx^2, dy^2
    int64_t nonfinite;
};

MTR_HD inline void rank_accumulate(RankSums& r, const PairCount& c, int64_t n, bool finite) {
    const int64_t dx = 2 * (int64_t)c.less_x + (int64_t)c.equal_x - n, dy = 2 * (int64_t)c.less_y + (int64_t)c.equal_y - n;
    r.s2 += c.s;
    r.tx += (int64_t)c.equal_x - 1;
    r.ty += (int64_t)c.equal_y - 1;
    r.dxy += dx * dy;
    r.dxx += dx * dx;
    r.dyy += dy * dy;
    r.nonfinite += finite ? 0 : 1;
}

// not `v - v == 0`: where v is a product, a compiler that contracts turns the difference into fma(a, b, -v), the product's
// rounding error, which is not zero for a finite v
MTR_HD inline bool is_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }
MTR_HD inline double quiet_nan() { return (double)NAN; }

// out[K_COUNT].  krcc is S / sqrt((n0 - n1) (n0 - n2)) evaluated as the host yardstick (head_train.kendall_tau_b) evaluates it:
// one product of two exactly converted integers, one square root, one division.
MTR_HD inline void rank_finish(const RankSums& r, int64_t n, double* out) {
    const int64_t n0 = n * (n - 1) / 2, n1 = r.tx / 2, n2 = r.ty / 2, S = r.s2 / 2;
    const double den = sqrt((double)(n0 - n1) * (double)(n0 - n2));
    const double rden = sqrt((double)r.dxx * (double)r.dyy);
    const bool bad = r.nonfinite != 0;
    out[K_KRCC] = (!bad && den > 0) ? (double)S / den : quiet_nan();
    out[K_SRCC] = (!bad && rden > 0) ? (double)r.dxy / rden : quiet_nan();
    out[K_S] = (double)S;
    out[K_N1] = (double)n1;
    out[K_N2] = (double)n2;
    out[K_N0] = (double)n0;
    out[K_NONFINITE] = (double)r.nonfinite;
    out[7] = 0.0;
}

// ---- the logistic model ---------------------------------------------------------------------------------------------------
// The 15 sums of one evaluation: J^T J (upper triangle, row-major), J^T r and r^T r, with r = f(x) - y.
struct Sums {
    double a[10], g[4], c;
};
constexpr int kSums = 15;

MTR_HD inline void sums_zero(Sums& s) {
    for (int k = 0; k < 10; ++k) s.a[k] = 0;
    for (int k = 0; k < 4; ++k) s.g[k] = 0;
    s.c = 0;
}

MTR_HD inline void sums_add(Sums& s, const Sums& o) {
    for (int k = 0; k < 10; ++k) s.a[k] += o.a[k];
    for (int k = 0; k < 4; ++k) s.g[k] += o.g[k];
    s.c += o.c;
}

MTR_HD inline double model(const double p[4], double x) {
    return p[1] + (p[0] - p[1]) / (1.0 + exp(-((x - p[2]) / fabs(p[3]))));
}

// f and df/dp at one x.  L = 1 / (1 + exp(-z)), z = (x - b3) / |b4|:  df/db1 = L, df/db2 = 1 - L,
// df/db3 = -(b1 - b2) L (1 - L) / |b4|, df/db4 = -(b1 - b2) L (1 - L) z sign(b4) / |b4|.
MTR_HD inline double model_row(const double p[4], double x, double J[4]) {
    const double s = fabs(p[3]);
    const double z = (x - p[2]) / s;
    const double L = 1.0 / (1.0 + exp(-z));
    const double w = (p[0] - p[1]) * L * (1.0 - L) / s;
    J[0] = L;
    J[1] = 1.0 - L;
    J[2] = -w;
    J[3] = (w == 0.0) ? 0.0 : -w * z * (p[3] < 0 ? -1.0 : 1.0);   // a saturated tail: 0, not 0 * a huge z
    return p[1] + (p[0] - p[1]) * L;
}

MTR_HD inline void sums_row(Sums& s, const double p[4], double x, double y) {
    double J[4];
    const double r = model_row(p, x, J) - y;
    int k = 0;
    for (int i = 0; i < 4; ++i)
        for (int j = i; j < 4; ++j) s.a[k++] += J[i] * J[j];
    for (int i = 0; i < 4; ++i) s.g[i] += J[i] * r;
    s.c += r * r;
}

MTR_HD inline int tri(int i, int j) {   // index of (i, j), i <= j, in the packed upper triangle of a 4x4
    return i * 4 - i * (i - 1) / 2 + (j - i);
}

// (A + lambda diag(A)) d = -g by Cholesky on the matrix scaled to a unit diagonal (Marquardt's scaling).  false when a
// column vanishes or a pivot is not positive: the caller raises lambda.
MTR_HD inline bool damped_solve(const Sums& s, double lambda, double d[4]) {
    double sc[4], M[4][4], b[4];
    for (int i = 0; i < 4; ++i) {
        const double dii = s.a[tri(i, i)];
        if (!(dii > 0.0) || !is_finite(dii)) return false;
        sc[i] = 1.0 / sqrt(dii);
    }
    for (int i = 0; i < 4; ++i) {
        for (int j = i; j < 4; ++j) M[i][j] = M[j][i] = s.a[tri(i, j)] * sc[i] * sc[j];
        M[i][i] = 1.0 + lambda;
        b[i] = -s.g[i] * sc[i];
    }
    for (int j = 0; j < 4; ++j) {   // M = L L^T, L in the lower triangle
        double v = M[j][j];
        for (int k = 0; k < j; ++k) v -= M[j][k] * M[j][k];
        if (!(v > 1e-14)) return false;
        M[j][j] = sqrt(v);
        for (int i = j + 1; i < 4; ++i) {
            double w = M[i][j];
            for (int k = 0; k < j; ++k) w -= M[i][k] * M[j][k];
            M[i][j] = w / M[j][j];
        }
    }
    for (int i = 0; i < 4; ++i) {
        double v = b[i];
        for (int k = 0; k < i; ++k) v -= M[i][k] * b[k];
        b[i] = v / M[i][i];
    }
    for (int i = 3; i >= 0; --i) {
        double v = b[i];
        for (int k = i + 1; k < 4; ++k) v -= M[k][i] * b[k];
        b[i] = v / M[i][i];
    }
    for (int i = 0; i < 4; ++i) {
        d[i] = b[i] * sc[i];
        if (!is_finite(d[i])) return false;
    }
    return true;
}

// The optimiser's state between evaluations.  Protocol: lm_begin sets `trial`; the caller evaluates the 15 sums there and
// hands them to lm_advance, which either sets the next `trial` (true) or ends the fit (false).
struct Lm {
    double p[4], trial[4], p0[4];
    Sums cur;
    double lambda, cost0;
    int iterations, converged, started;
};

MTR_HD inline void lm_begin(Lm& m, const double p0[4]) {
    for (int i = 0; i < 4; ++i) m.p[i] = m.trial[i] = m.p0[i] = p0[i];
    sums_zero(m.cur);
    m.lambda = kLambda0;
    m.cost0 = 0;
    m.iterations = 0;
    m.converged = 0;
    m.started = 0;
}

// Stopping rule at the current point, on the undamped (Gauss-Newton) step d: the model predicts a relative reduction of the
// cost of at most ftol, or the step is at most xtol of the parameter vector in the scaled norm - MINPACK's two tests taken at
// its limit of a vanishing LM parameter, so a step that is short only because the damping is high never ends the fit.
MTR_HD inline bool lm_at_minimum(const Lm& m) {
    if (m.cur.c == 0.0) return true;
    double d[4];
    if (!damped_solve(m.cur, 0.0, d)) return false;
    double pred = 0, dn = 0, xn = 0;
    for (int i = 0; i < 4; ++i) {
        pred -= m.cur.g[i] * d[i];     // cost(p) - model(p + d) = -g.d at the Gauss-Newton step
        dn += m.cur.a[tri(i, i)] * d[i] * d[i];
        xn += m.cur.a[tri(i, i)] * m.p[i] * m.p[i];
    }
    return pred <= kTol * m.cur.c || sqrt(dn) <= kTol * sqrt(xn);
}

MTR_HD inline bool lm_advance(Lm& m, const Sums& at_trial) {
    if (!m.started) {
        m.started = 1;
        m.cur = at_trial;
        m.cost0 = at_trial.c;
        if (!is_finite(at_trial.c)) return false;
    } else {
        ++m.iterations;
        if (is_finite(at_trial.c) && at_trial.c < m.cur.c) {   // step acceptance: the cost went down
            for (int i = 0; i < 4; ++i) m.p[i] = m.trial[i];
            m.cur = at_trial;
            m.lambda = m.lambda * 0.1 > kLambdaMin ? m.lambda * 0.1 : kLambdaMin;
        } else {
            m.lambda *= 10.0;
        }
    }
    if (lm_at_minimum(m)) {
        m.converged = 1;
        return false;
    }
    if (m.iterations >= kMaxIter) return false;
    for (;;) {
        if (m.lambda > kLambdaMax) return false;
        double d[4];
        bool ok = damped_solve(m.cur, m.lambda, d);
        if (ok) {
            bool moved = false;
            for (int i = 0; i < 4; ++i) {
                m.trial[i] = m.p[i] + d[i];
                ok = ok && is_finite(m.trial[i]);
                moved = moved || m.trial[i] != m.p[i];
            }
            if (ok && !moved) return false;   // the step is below the spacing of the parameters: nothing left to try
            if (ok) return true;
        }
        m.lambda *= 10.0;
    }
}

// out[O_POPT .. O_COST] and O_P0 from a finished fit
MTR_HD inline void lm_report(const Lm& m, double* out) {
    for (int i = 0; i < 4; ++i) {
        out[O_POPT + i] = m.p[i];
        out[O_P0 + i] = m.p0[i];
    }
    out[O_ITER] = (double)m.iterations;
    out[O_CONVERGED] = (double)m.converged;
    out[O_COST0] = m.cost0;
    out[O_COST] = m.cur.c;
}

// plcc from centred sums (syy, sff, syf of y - mean(y) and f - mean(f)); nan for a constant vector
MTR_HD inline double pearson_from_centred(double syy, double sff, double syf) {
    const double den = sqrt(syy) * sqrt(sff);
    return den > 0 ? syf / den : quiet_nan();
}

}  // namespace mtr
