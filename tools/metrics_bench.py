"""Times the correlation metrics (csrc/metrics.hip) and writes profiles/metrics_bench.json.

    python tools/metrics_bench.py [--out profiles/metrics_bench.json] [--no-protocol]

For n in {96, 240, 1200, 7400, 28000}: ms per call of the pair pass (relax_metrics_kendall) and of the full
relax_metrics_correlation, results left in device memory so a call only enqueues - the median of `--repeats` timed runs of
`--steps` back-to-back calls after a warm-up, HIP events around the run (min / max over the repeats are the spread).  Beside
them the host yardsticks on the same vectors, wall time of one call each: head_train.kendall_tau_b (the n x n numpy form; not
run where its temporaries pass --host-limit-gb, and marked so), scipy.stats.kendalltau and scipy.optimize.curve_fit.  Last:
the wall time of one holdout_protocol on a KoNViD-shaped synthetic set (1200 rows, F = 35203).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import relax_vqa_amd  # noqa: E402,F401
from relax_vqa_amd import head_train, metrics  # noqa: E402
from relax_vqa_amd.engine import RelaxEngine  # noqa: E402

SIZES = (96, 240, 1200, 7400, 28000)


def timed(fn, steps, repeats, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / steps)
    return {"median_ms": float(np.median(out)), "min_ms": float(min(out)), "max_ms": float(max(out)), "repeats": repeats, "steps": steps}


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def vectors(n):
    rng = np.random.RandomState(n)
    y_true = 1.0 + 4.0 * rng.uniform(size=n)
    y_pred = 0.3 * (y_true + 0.6 * rng.standard_normal(n)) + 1.6
    return y_true, y_pred


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_bench.json"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-limit-gb", type=float, default=8.0, help="skip head_train.kendall_tau_b where its temporaries exceed this")
    ap.add_argument("--no-protocol", action="store_true")
    ap.add_argument("--protocol-repeats", type=int, default=3)
    args = ap.parse_args()
    eng = RelaxEngine(0)
    result = {"device": torch.cuda.get_device_name(0), "sizes": {}}
    try:
        from scipy.stats import kendalltau
        import metrics_cases as MC
    except ImportError:
        kendalltau = MC = None
    for n in SIZES:
        y_true, y_pred = vectors(n)
        yt, yp = torch.as_tensor(y_true).to(eng.device), torch.as_tensor(y_pred).to(eng.device)
        out_k = torch.empty(metrics.KENDALL_COUNT, dtype=torch.float64, device=eng.device)
        out_c = torch.empty(metrics.OUT_COUNT, dtype=torch.float64, device=eng.device)
        row = {"pair_pass": timed(lambda: metrics.kendall_async(eng, yt, yp, out_k), args.steps, args.repeats, args.warmup),
               "correlation_metrics": timed(lambda: metrics.correlation_metrics_async(eng, yt, yp, out_c), args.steps, args.repeats,
                                            args.warmup)}
        row["lm_iterations"] = int(out_c[8].item())
        row["with_host_read_wall_ms"] = float(np.median([wall(lambda: eng.correlation_metrics(yt, yp)) for _ in range(5)]))
        temporaries_gb = 6 * 8.0 * n * n / 2 ** 30    # the two sign matrices, the index pair and their gathers
        if temporaries_gb <= args.host_limit_gb:
            row["host_kendall_tau_b_wall_ms"] = float(np.median([wall(lambda: head_train.kendall_tau_b(y_true, y_pred)) for _ in range(3)]))
        else:
            row["host_kendall_tau_b_wall_ms"] = None
            row["host_kendall_tau_b_skipped"] = f"about {temporaries_gb:.0f} GB of n x n temporaries"
        if kendalltau is not None:
            row["scipy_kendalltau_wall_ms"] = float(np.median([wall(lambda: kendalltau(y_true, y_pred)) for _ in range(3)]))
            row["scipy_curve_fit_wall_ms"] = float(np.median([wall(lambda: MC.scipy_fit(y_true, y_pred)) for _ in range(3)]))
        result["sizes"][str(n)] = row
        print(n, json.dumps(row), flush=True)
    if not args.no_protocol:
        n, F = 1200, 35203
        rng = np.random.RandomState(0)
        x = torch.as_tensor(rng.uniform(0, 1, size=(n, F)).astype(np.float32)).to(eng.device)
        mos = (1 + 4 * rng.uniform(size=n)).astype(np.float64)
        t0 = time.perf_counter()
        res = eng.holdout_protocol(x, mos, dict(n_splits=10, epochs=20), n_repeats=args.protocol_repeats)
        torch.cuda.synchronize()
        result["holdout_protocol"] = {"rows": n, "features": F, "n_repeats": args.protocol_repeats, "n_splits": 10, "epochs": 20,
                                      "wall_s": time.perf_counter() - t0, "wall_s_per_repeat": (time.perf_counter() - t0) / args.protocol_repeats,
                                      "median_index": res["median_index"]}
        print(json.dumps(result["holdout_protocol"]), flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
