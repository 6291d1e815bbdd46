"""The cases of the metrics checks, shared by the CPU tests, the sanitizer driver and the GPU tests (numpy only).

Rank statistics: n in {2, 3, 30, 240, 1200} x {no ties, heavy ties (one decimal), one constant vector, monotone, anti-monotone}.
Logistic fit, well-conditioned: targets 1 + 4 q and 100 q (q uniform), predictions = target + Gaussian noise of 0.05 / 0.3 of
half the range, raw or compressed by 0.3 and shifted, n in {240, 1200, 7000}, five seeds each (120 cases).
Logistic fit, ill-conditioned: n = 30 with the same noises, and noise 0.8 / 1.2 of half the range at n in {240, 1200}."""
import numpy as np

RANK_SIZES = (2, 3, 30, 240, 1200)
RANK_KINDS = ("no_ties", "heavy_ties", "constant", "monotone", "anti_monotone")
FIT_SIZES = (240, 1200, 7000)
SEEDS = (0, 1, 2, 3, 4)
FTOL = 1.49e-8


def rank_case(n, kind, seed=0):
    rng = np.random.RandomState(1000 * n + seed)
    x = rng.standard_normal(n)
    y = 0.6 * x + 0.8 * rng.standard_normal(n)
    if kind == "heavy_ties":
        x, y = np.round(x, 1), np.round(y, 1)
    elif kind == "constant":
        y = np.full(n, 2.5)
    elif kind == "monotone":
        y = np.exp(x)
    elif kind == "anti_monotone":
        y = -3.0 * x + 1.0
    return x.astype(np.float64), np.asarray(y, dtype=np.float64)


def rank_cases():
    return [(f"{kind}-n{n}", n, kind) for n in RANK_SIZES for kind in RANK_KINDS]


def fit_case(n, scale, noise, compressed, seed):
    """(y_true, y_pred): scale 'mos5' -> 1 + 4 q, 'mos100' -> 100 q; noise as a fraction of half the target range."""
    rng = np.random.RandomState(seed * 7919 + n)
    q = rng.uniform(size=n)
    lo, hi = (1.0, 5.0) if scale == "mos5" else (0.0, 100.0)
    y_true = lo + (hi - lo) * q
    y_pred = y_true + noise * 0.5 * (hi - lo) * rng.standard_normal(n)
    if compressed:
        y_pred = 0.3 * y_pred + 0.4 * (hi - lo)
    return y_true, y_pred


def well_conditioned():
    return [(f"{scale}-noise{noise}-{'compressed' if comp else 'raw'}-n{n}-s{seed}", (n, scale, noise, comp, seed))
            for n in FIT_SIZES for scale in ("mos5", "mos100") for noise in (0.05, 0.3) for comp in (False, True) for seed in SEEDS]


def ill_conditioned():
    small = [(30, scale, noise, comp, seed) for scale in ("mos5", "mos100") for noise in (0.05, 0.3) for comp in (False, True)
             for seed in SEEDS[:2]]
    noisy = [(n, scale, noise, comp, seed) for n in (240, 1200) for scale in ("mos5", "mos100") for noise in (0.8, 1.2)
             for comp in (False, True) for seed in SEEDS[:2]]
    return [(f"{a[1]}-noise{a[2]}-{'compressed' if a[3] else 'raw'}-n{a[0]}-s{a[4]}", a) for a in small + noisy]


def logistic(x, b1, b2, b3, b4):
    """The 4-parameter logistic, restated from its formula."""
    return b2 + (b1 - b2) / (1.0 + np.exp(-(x - b3) / np.abs(b4)))


def scipy_fit(y_true, y_pred):
    """scipy.optimize.curve_fit from the reference's p0 -> (popt, rmse, plcc)."""
    import warnings
    from scipy.optimize import curve_fit
    from scipy.stats import pearsonr
    p0 = [np.max(y_true), np.min(y_true), np.mean(y_pred), 0.5]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        popt, _ = curve_fit(logistic, y_pred, y_true, p0=p0, maxfev=100000000)
    fitted = logistic(y_pred, *popt)
    return popt, float(np.sqrt(np.mean((y_true - fitted) ** 2))), float(pearsonr(y_true, fitted)[0])


def stopping_rule_holds(y_true, y_pred, p, slack):
    """The stopping rule of metrics_core.h evaluated independently in numpy at p: the Gauss-Newton step predicts a relative
    cost reduction <= ftol, or is <= xtol of p in the column-scaled norm."""
    s = abs(p[3])
    z = (y_pred - p[2]) / s
    L = 1.0 / (1.0 + np.exp(-z))
    w = (p[0] - p[1]) * L * (1 - L) / s
    J = np.stack([L, 1 - L, -w, -w * z * np.sign(p[3])], axis=1)
    r = p[1] + (p[0] - p[1]) * L - y_true
    d = np.linalg.lstsq(J, -r, rcond=None)[0]
    cost = float(r @ r)
    pred = cost - float(np.sum((r + J @ d) ** 2))
    col = np.sqrt((J * J).sum(0))
    return pred <= slack * FTOL * cost or np.linalg.norm(col * d) <= slack * FTOL * np.linalg.norm(col * p)
