"""ctypes binding of the host build of csrc/metrics_core.h (csrc/metrics_host.cpp), for the CPU tests and as the yardstick of
the GPU tests: host_metrics(y_true, y_pred) runs the pair pass, the rank finish and the Levenberg-Marquardt fit in one thread.

Run as a script INSIDE a subprocess with libasan preloaded (tests/test_metrics_sanitized.py) it drives the sanitizer build
(librelax_metrics_san.so) through the rank, well-conditioned and ill-conditioned cases of tests/metrics_cases.py.  Inputs and
outputs sit in malloc'd buffers of exactly their size, so a read or write outside them is a sanitizer report."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "relax-vqa_amd", "csrc")
OUT_COUNT, KENDALL_COUNT = 17, 8
_libs = {}


def load(sanitized=False):
    name = "librelax_metrics_san.so" if sanitized else "librelax_metrics_host.so"
    if name not in _libs:
        if not sanitized:   # the sanitizer build is made by its test, outside the process that preloads libasan
            subprocess.run(["make", "-C", CSRC, name], check=True, capture_output=True)   # a no-op when it is up to date
        lib = C.CDLL(os.path.join(CSRC, name))
        lib.relax_metrics_host.restype = C.c_int
        lib.relax_metrics_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5
        _libs[name] = lib
    return _libs[name]


def host_metrics(y_true, y_pred, ranks=True, fit=True, p0=None, want_counts=False, sanitized=False, exact_buffers=False):
    """-> dict with the names RelaxEngine.correlation_metrics uses (+ 'S', 'n1', 'n2', 'n0', 'counts', 'y_pred_logistic')."""
    lib = load(sanitized)
    y_true = np.ascontiguousarray(y_true, dtype=np.float64).reshape(-1)
    y_pred = np.ascontiguousarray(y_pred, dtype=np.float64).reshape(-1)
    n = y_true.size
    assert y_pred.size == n
    out_k = np.full(KENDALL_COUNT, np.nan)
    out = np.full(OUT_COUNT, np.nan)
    fitted = np.full(n, np.nan)
    counts = np.zeros((5, n), dtype=np.int32) if want_counts else None
    start = None if p0 is None else np.ascontiguousarray(p0, dtype=np.float64)
    flags = (1 if ranks else 0) | (2 if fit else 0)
    if exact_buffers:
        libc = C.CDLL(None)
        libc.malloc.restype = C.c_void_p
        libc.malloc.argtypes = [C.c_size_t]
        libc.free.argtypes = [C.c_void_p]
        bufs = [libc.malloc(max(a.nbytes, 1)) for a in (y_true, y_pred, out_k, out, fitted)]
        cbuf = libc.malloc(max(counts.nbytes, 1)) if want_counts else None
        C.memmove(bufs[0], y_true.ctypes.data, y_true.nbytes)
        C.memmove(bufs[1], y_pred.ctypes.data, y_pred.nbytes)
        try:
            rc = lib.relax_metrics_host(bufs[0], bufs[1], n, flags, start.ctypes.data if start is not None else None, bufs[2], cbuf,
                                        bufs[3], bufs[4])
            if rc == 0:
                for a, b in zip((out_k, out, fitted), bufs[2:]):
                    C.memmove(a.ctypes.data, b, a.nbytes)
                if want_counts:
                    C.memmove(counts.ctypes.data, cbuf, counts.nbytes)
        finally:
            for b in bufs + ([cbuf] if cbuf else []):
                libc.free(b)
    else:
        rc = lib.relax_metrics_host(y_true.ctypes.data, y_pred.ctypes.data, n, flags, start.ctypes.data if start is not None else None,
                                    out_k.ctypes.data, counts.ctypes.data if want_counts else None, out.ctypes.data, fitted.ctypes.data)
    if rc != 0:
        raise ValueError(f"relax_metrics_host refused n = {n}")
    res = {}
    if ranks:
        res.update(krcc=float(out_k[0]), srcc=float(out_k[1]), S=int(out_k[2]), n1=int(out_k[3]), n2=int(out_k[4]), n0=int(out_k[5]),
                   nonfinite=int(out_k[6]))
    if fit:
        res.update(plcc=float(out[0]), rmse=float(out[1]), popt=out[4:8].copy(), beta=out[13:17].copy(), iterations=int(out[8]),
                   converged=bool(out[9] == 1.0), cost0=float(out[10]), cost=float(out[11]), nonfinite=int(out[12]),
                   y_pred_logistic=fitted)
    if want_counts:
        res["counts"] = counts
    return res


def _main():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import metrics_cases as MC
    done = 0
    for _, n, kind in MC.rank_cases():
        x, y = MC.rank_case(n, kind)
        r = host_metrics(x, y, fit=False, want_counts=True, sanitized=True, exact_buffers=True)
        assert r["n0"] == n * (n - 1) // 2 and int(r["counts"][4].sum()) == 2 * r["S"], (n, kind)
        done += 1
    for _, args in MC.well_conditioned() + MC.ill_conditioned():
        y_true, y_pred = MC.fit_case(*args)
        r = host_metrics(y_true, y_pred, ranks=args[0] <= 1200, sanitized=True, exact_buffers=True)
        assert np.isfinite(r["popt"]).all() and np.isfinite(r["rmse"]) and r["cost"] <= r["cost0"], args
        done += 1
    bad = np.array([1.0, np.nan, 3.0, np.inf])
    r = host_metrics(bad, np.arange(4.0), sanitized=True, exact_buffers=True)
    assert r["nonfinite"] == 2 and np.isnan(r["krcc"]) and np.isnan(r["rmse"])
    print(f"METRICS_SANITIZED_OK {done + 1}")


if __name__ == "__main__":
    _main()
