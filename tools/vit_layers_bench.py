"""The ViT layer-stack taps on the MI355X (relax_vit_intermediate_layers, csrc/vit_layers.hip), device events after a warm-up, median of 7,
one card, one process:

  - the fused kernel alone (vit_norm_token_stats: LayerNorm + CLS row + token statistics of a tap, no normed tokens in HBM) against the two
    launches it replaces (layernorm_rows<0> into a buffer, then vit_token_stats), alternating in the same run on the same tensors, ViT-B rows:
    197 tokens x 256 images and 785 tokens x 64 images.  Each sample times `inner` back-to-back launches over a ring of input buffers larger
    than the 256 MB Infinity Cache ("cold": X comes from HBM, as the bytes of a stream the forward wrote long ago would), and again on one
    buffer ("warm": X is where the fc2 GEMM that has just written it left it).  GB/s counts the compulsory traffic alone - X once - against the
    6.29 TB/s copy rate.  (relax_op_token_stats has no row offset: the pair's second launch reads all ntok rows where the forward's reads
    ntok - 1, 0.5 % more at 197 tokens);
  - what the fused kernel fetches: one `rocprofv3 --pmc FETCH_SIZE` child of its own (counters only, no tracing), run before this process
    opens the GPU, two dispatches of each of the three kernels at 197 x 256;
  - the cost of taps: a pooled ViT-B pass of 256 images under f16x2 and fp32 with n = 1, 4, 12 cls + pooled taps against
    vit_features(pooled=True), alternating, as ms and percent.

  python tools/vit_layers_bench.py [--reps 7] [--no-pmc] [--out profiles/vit_layers_bench.json]

Synthetic weights and random inputs: the timing does not depend on the values."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import relax_vqa_amd  # noqa: E402,F401
from relax_vqa_amd import synth  # noqa: E402
from relax_vqa_amd.engine import RelaxEngine  # noqa: E402

DIM = 768
EPS = 1e-6
COPY_RATE_GBS = 6290.0
FAULT_STATUS = (134, 139, 124, 137, -6, -11, -9)
KERNEL_SHAPES = [("197x256", 197, 256), ("785x64", 785, 64)]


class _Ops:
    """the three launches on preallocated buffers, through the C-ABI (no allocation inside a timed window)"""

    def __init__(self, eng, ntok, n_img, buffers):
        g = torch.Generator().manual_seed(ntok)
        self.eng, self.ntok, self.n = eng, ntok, n_img
        self.xs = [(torch.randn((n_img, ntok, DIM), generator=g) * 2 + 1).cuda() for _ in range(buffers)]
        self.gamma = (1 + 0.1 * torch.randn(DIM, generator=g)).cuda()
        self.beta = (0.1 * torch.randn(DIM, generator=g)).cuda()
        self.y = torch.empty_like(self.xs[0])
        self.cls = torch.empty((n_img, DIM), dtype=torch.float32, device="cuda")
        self.pooled = torch.empty((n_img, 3 * DIM), dtype=torch.float32, device="cuda")
        self.pooled_pair = torch.empty_like(self.pooled)

    def fused(self, x):
        e = self.eng
        e._check(e.lib.relax_op_vit_norm_token_stats(e.h, x.data_ptr(), self.gamma.data_ptr(), self.beta.data_ptr(), EPS, self.cls.data_ptr(),
                                                     self.pooled.data_ptr(), self.n, self.ntok, DIM, None), "relax_op_vit_norm_token_stats")

    def pair(self, x):
        e = self.eng
        e._check(e.lib.relax_op_layernorm(e.h, x.data_ptr(), self.gamma.data_ptr(), self.beta.data_ptr(), self.y.data_ptr(), self.n * self.ntok,
                                          DIM, EPS, None), "relax_op_layernorm")
        e._check(e.lib.relax_op_token_stats(e.h, self.y.data_ptr(), self.pooled_pair.data_ptr(), self.n, self.ntok, DIM, None),
                 "relax_op_token_stats")


def pmc_step():
    """the rocprofv3 target: two dispatches of each kernel at 197 tokens x 256 images"""
    ops = _Ops(RelaxEngine(0), 197, 256, 1)
    for _ in range(2):
        ops.fused(ops.xs[0])
        ops.pair(ops.xs[0])
    torch.cuda.synchronize()


def fetch_sizes():
    """-> {kernel: FETCH_SIZE of each dispatch as the tool reports it} from one counters-only child"""
    d = tempfile.mkdtemp(prefix="vit_layers_pmc_")
    cmd = ["rocprofv3", "--pmc", "FETCH_SIZE", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--pmc-step"]
    try:
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired:
        raise SystemExit("vit_layers_bench: the counter child ran into its time limit")
    if res.returncode in FAULT_STATUS:   # a fault, an abort or a time limit on the card: nothing more is started on it
        raise SystemExit(f"vit_layers_bench: the counter child ended with status {res.returncode}: {res.stderr[-300:]}")
    files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
    if res.returncode != 0 or not files:
        return {"not_measured": f"rocprofv3 rc {res.returncode}: {res.stderr[-300:]}"}
    out = {}
    for r in csv.DictReader(open(files[0])):
        name = r.get("Kernel_Name", "")
        if r.get("Counter_Name") != "FETCH_SIZE":
            continue
        for key in ("vit_norm_token_stats", "layernorm_rows", "vit_token_stats"):
            if key in name:
                out.setdefault(key, []).append(float(r["Counter_Value"]))
    x_bytes = 256 * 197 * DIM * 4
    return {"fetch_size_per_dispatch": out, "x_bytes": x_bytes, "unit": "as rocprofv3 reports FETCH_SIZE (KB in its derived-metric definition)",
            "note": "the counter sits on the L2's memory side: Infinity Cache hits are counted; 16-byte-per-lane streaming reads are tallied at half "
                    "their bytes on gfx950, the 4-byte-per-lane reads of the later passes are uncalibrated"}


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _stats(ts):
    med = float(np.median(ts))
    return {"ms_median": round(med, 4), "ms_min": round(float(np.min(ts)), 4), "ms_max": round(float(np.max(ts)), 4),
            "spread_pct": round(100.0 * (float(np.max(ts)) - float(np.min(ts))) / med, 2)}


def _time_alternating(fns, reps, warmup=2):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(_event_ms(fn))
    return {k: _stats(v) for k, v in ts.items()}


def kernel_alone(eng, reps):
    out = {}
    for label, ntok, n_img in KERNEL_SHAPES:
        x_bytes = n_img * ntok * DIM * 4
        buffers = -(-(320 << 20) // x_bytes) + 1          # a ring past the Infinity Cache
        ops = _Ops(eng, ntok, n_img, buffers)
        inner = 2 * buffers
        rec = {"images": n_img, "tokens": ntok, "x_bytes": x_bytes, "ring_buffers": buffers, "launches_per_sample": inner}
        for mode, ring in (("cold", ops.xs), ("warm", ops.xs[:1])):
            def run(fn, ring=ring):
                for i in range(inner):
                    fn(ring[i % len(ring)])
            t = _time_alternating({"fused": lambda: run(ops.fused), "pair": lambda: run(ops.pair)}, reps)
            for k in t:
                us = 1e3 * t[k]["ms_median"] / inner
                t[k]["us_per_launch"] = round(us, 2)
                t[k]["compulsory_gbs"] = round(x_bytes / (us * 1e-6) / 1e9, 1)
                t[k]["of_copy_rate_pct"] = round(100.0 * t[k]["compulsory_gbs"] / COPY_RATE_GBS, 1)
            t["fused_over_pair_pct"] = round(100.0 * (t["fused"]["ms_median"] / t["pair"]["ms_median"] - 1.0), 2)
            t["faster_by_more_than_the_spread"] = bool(
                t["fused"]["ms_median"] < t["pair"]["ms_median"] and
                (t["pair"]["ms_median"] - t["fused"]["ms_median"]) / t["pair"]["ms_median"] * 100.0 > max(t["fused"]["spread_pct"], t["pair"]["spread_pct"]))
            rec[mode] = t
        ops.fused(ops.xs[0])
        ops.pair(ops.xs[0])
        torch.cuda.synchronize()
        ref = eng.op_token_stats(ops.y[:, 1:].contiguous())
        rec["bit_equal_to_the_forward's_pair"] = bool(torch.equal(ops.pooled, ref) and torch.equal(ops.cls, ops.y[:, 0]))
        out[label] = rec
        del ops
        torch.cuda.empty_cache()
    return out


def tap_cost(eng, reps):
    eng.load_vit(synth.vit_state_dict("vit_base"), "vit_base")
    n_img = 256
    x = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (n_img, 224, 224, 3), dtype=np.uint8)).cuda()
    pooled = torch.empty((n_img, 3 * DIM), dtype=torch.float32, device="cuda")
    taps_cls = torch.empty((12, n_img, DIM), dtype=torch.float32, device="cuda")
    taps_pooled = torch.empty((12, n_img, 3 * DIM), dtype=torch.float32, device="cuda")
    out = {"images": n_img}
    for precision in ("f16x2", "fp32"):
        eng.set_precision(precision)

        def features():
            eng._check(eng.lib.relax_vit_features(eng.h, x.data_ptr(), n_img, None, pooled.data_ptr(), None), "relax_vit_features")

        def tapped(n):
            eng._check(eng.lib.relax_vit_intermediate_layers(eng.h, x.data_ptr(), n_img, 224, 224, n, None, taps_cls.data_ptr(),
                                                             taps_pooled.data_ptr(), None), "relax_vit_intermediate_layers")

        t = _time_alternating({"vit_features": features, "n=1": lambda: tapped(1), "n=4": lambda: tapped(4), "n=12": lambda: tapped(12)}, reps)
        base = t["vit_features"]["ms_median"]
        for k in ("n=1", "n=4", "n=12"):
            t[k]["over_vit_features_ms"] = round(t[k]["ms_median"] - base, 3)
            t[k]["over_vit_features_pct"] = round(100.0 * (t[k]["ms_median"] / base - 1.0), 2)
        tapped(1)
        features()
        torch.cuda.synchronize()
        t["n=1_pooled_bit_equal"] = bool(torch.equal(taps_pooled[0], pooled))
        out[precision] = t
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-pmc", action="store_true")
    ap.add_argument("--pmc-step", action="store_true")
    args = ap.parse_args()
    if args.pmc_step:
        return pmc_step()
    fetch = {"not_measured": "--no-pmc"} if args.no_pmc else fetch_sizes()   # the child first: this process has not opened the GPU yet
    if not torch.cuda.is_available():
        raise SystemExit("vit_layers_bench: no GPU - nothing is measured without one")
    eng = RelaxEngine(0)
    out = {"model": "vit_base/16", "reps": args.reps, "copy_rate_gbs": COPY_RATE_GBS, "fetch": fetch}
    out["kernel_alone"] = kernel_alone(eng, args.reps)
    out["tap_cost"] = tap_cost(eng, args.reps)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
