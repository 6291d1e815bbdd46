"""The fragment stage (csrc/fragment.hip) at patch sizes 8, 16 and 32 on the MI355X, timed with device events after a warm-up.

Per shape (540p, 1080p, 2160p; T = 32 pairs) and patch size, all (224 / P)^2 slots selected, ms per call as median / min / max over
--repeats repeats of --calls back-to-back calls of the C entry point (buffers allocated once, outside the timing):
  whole          relax_fragment_pairs_ex with both canvases: score + select + two gathers
  score          the score kernel alone, from the library's own event span around it (relax_profile_read kind 1), beside the bytes
                 it reads and writes and the fraction of the 6.29 TB/s copy rate that makes
  score_select   the same call without canvases (score + select)
  select         score_select - score (derived: the selection kernel has no entry point of its own)
  gather         relax_gather_patches_ex on the first frames with the selected positions: one of the call's two gathers
For P = 8 the record says which of score and select is the larger one.

--parent-lib PATH: a librelax_hip.so built from the parent commit.  The script then starts itself once more as a child process on
that library with --old-entry, which times the P = 16 case through relax_fragment_pairs (the entry point without geometry
arguments, the only one the parent has) on the same card in the same session, and records per shape
  parent_16 / new_16 whole-call times, spread_ms = the larger of the two runs' max - min, new_not_slower = new <= parent + spread.

  python tools/fragment_geometry_bench.py [--pairs 32] [--repeats 7] [--calls 5] [--parent-lib PATH] [--out profiles/fragment_geometry_bench.json]

Random frames: the timing of score and gather does not depend on the values; the selection's does only through the number of
candidates of its second radix level."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import relax_vqa_amd  # noqa: E402,F401
from relax_vqa_amd import _lib  # noqa: E402

COPY_TBPS = 6.29
SHAPES = (("540p", 540, 960), ("1080p", 1080, 1920), ("2160p", 2160, 3840))
TARGET = 224


class Lib:
    """the entry points this script needs, bound on any build of the library (the parent's has no *_ex symbols)"""

    def __init__(self, path):
        torch.zeros(1, device="cuda")     # the HIP context exists before the library touches it
        self.lib = C.CDLL(path)
        for name, (res, args) in _lib.PROTOTYPES.items():
            fn = getattr(self.lib, name, None)
            if fn is not None:
                fn.restype, fn.argtypes = res, args
        self.h = C.c_void_p()
        rc = self.lib.relax_create(0, C.byref(self.h))
        if rc != 0:
            raise RuntimeError(f"relax_create failed ({rc}): {self.lib.relax_last_error(None).decode()}")

    def check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {self.lib.relax_last_error(self.h).decode()}")

    def score_ms(self, fn, n):
        """ms per call of the score kernel over n calls of fn, from the library's span around it"""
        self.check(self.lib.relax_profile_enable(self.h, 1), "relax_profile_enable")
        for _ in range(n):
            fn()
        ms, work, cnt = C.c_double(), C.c_double(), C.c_int64()
        self.check(self.lib.relax_profile_read(self.h, 1, C.byref(ms), C.byref(work), C.byref(cnt)), "relax_profile_read")
        self.check(self.lib.relax_profile_enable(self.h, 0), "relax_profile_enable")
        return ms.value / max(cnt.value, 1)


def _time_ms(fn, repeats, calls, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / calls)
    return {"ms_median": round(float(np.median(ts)), 4), "ms_min": round(float(np.min(ts)), 4), "ms_max": round(float(np.max(ts)), 4)}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def measure(lib, args, patches, old_entry):
    out = {}
    for label, H, W in SHAPES:
        T = args.pairs
        frames = torch.randint(0, 256, (T, 2, H, W, 3), dtype=torch.uint8, device="cuda")
        fb = H * W * 3
        a, b = frames.data_ptr(), frames.data_ptr() + fb
        out[label] = {"T": T, "H": H, "W": W}
        for P in patches:
            slots = (TARGET // P) ** 2
            pos = torch.empty((T, slots, 2), dtype=torch.int32, device="cuda")
            cnt = torch.empty((T,), dtype=torch.int32, device="cuda")
            ori, diff = (torch.empty((T, TARGET, TARGET, 3), dtype=torch.uint8, device="cuda") for _ in range(2))

            def call(with_frags=True):
                fa, fd = (ori.data_ptr(), diff.data_ptr()) if with_frags else (None, None)
                if old_entry:
                    rc = lib.lib.relax_fragment_pairs(lib.h, a, b, 2 * fb, T, H, W, slots, pos.data_ptr(), cnt.data_ptr(), fa, fd, None, _stream())
                else:
                    rc = lib.lib.relax_fragment_pairs_ex(lib.h, a, b, 2 * fb, T, H, W, P, TARGET, slots, pos.data_ptr(), cnt.data_ptr(), fa, fd,
                                                         None, _stream())
                lib.check(rc, "relax_fragment_pairs")

            def gather():
                if old_entry:
                    rc = lib.lib.relax_gather_patches(lib.h, a, 2 * fb, T, H, W, pos.data_ptr(), cnt.data_ptr(), ori.data_ptr(), _stream())
                else:
                    rc = lib.lib.relax_gather_patches_ex(lib.h, a, 2 * fb, T, H, W, P, TARGET, pos.data_ptr(), cnt.data_ptr(), ori.data_ptr(),
                                                         _stream())
                lib.check(rc, "relax_gather_patches")

            rec = {"slots": slots, "patches_per_item": (H // P) * (W // P)}
            rec["whole"] = _time_ms(call, args.repeats, args.calls)
            rec["score_select"] = _time_ms(lambda: call(False), args.repeats, args.calls)
            rec["gather"] = _time_ms(gather, args.repeats, args.calls)
            score = lib.score_ms(lambda: call(False), args.repeats * args.calls)
            torch.cuda.synchronize()
            nbytes = 2.0 * T * (H // P) * P * (W // P) * P * 3 + 4.0 * T * (H // P) * (W // P)
            rec["score"] = {"ms": round(score, 4), "MB_moved": round(nbytes / 1e6, 1),
                            "fraction_of_copy_rate": round(nbytes / (score * 1e-3) / (COPY_TBPS * 1e12), 3)}
            rec["select"] = {"ms_derived": round(rec["score_select"]["ms_median"] - score, 4)}
            rec["larger_of_score_and_select"] = "select" if rec["select"]["ms_derived"] > score else "score"
            out[label][f"P{P}"] = rec
            print(label, f"P{P}", json.dumps(rec), file=sys.stderr, flush=True)
        del frames
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--lib", default=_lib.LIB_PATH)
    ap.add_argument("--old-entry", action="store_true", help="P = 16 alone, through relax_fragment_pairs / relax_gather_patches")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.old_entry:         # the child on the parent's library: one JSON line on stdout
        print(json.dumps(measure(Lib(args.lib), args, (16,), True)))
        return
    out = {"copy_rate_TBps": COPY_TBPS, "repeats": args.repeats, "calls_per_repeat": args.calls, "target_size": TARGET}
    parent = None
    if args.parent_lib:
        cmd = [sys.executable, os.path.abspath(__file__), "--old-entry", "--lib", os.path.abspath(args.parent_lib), "--pairs", str(args.pairs),
               "--repeats", str(args.repeats), "--calls", str(args.calls)]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if res.returncode != 0:
            raise RuntimeError(f"the run on the parent's library failed ({res.returncode}):\n{res.stderr[-2000:]}")
        parent = json.loads(res.stdout.strip().splitlines()[-1])
    out["shapes"] = measure(Lib(args.lib), args, (8, 16, 32), False)
    if parent is not None:
        out["parent_old_entry_point"] = parent
        cmp_ = {}
        for label, _, _ in SHAPES:
            new, old = out["shapes"][label]["P16"]["whole"], parent[label]["P16"]["whole"]
            spread = max(new["ms_max"] - new["ms_min"], old["ms_max"] - old["ms_min"])
            cmp_[label] = {"parent_16_ms": old["ms_median"], "new_16_ms": new["ms_median"], "spread_ms": round(spread, 4),
                           "new_not_slower": bool(new["ms_median"] <= old["ms_median"] + spread)}
        out["p16_against_parent"] = cmp_
        print(json.dumps(cmp_), file=sys.stderr, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    else:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
