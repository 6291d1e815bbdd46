"""Times the quality head's training step (csrc/head_train.hip) and writes profiles/head_train_bench.json.

    python tools/head_train_bench.py [--out profiles/head_train_bench.json] [--steps 200] [--no-fit]
    python tools/head_train_bench.py --optimizer adam          # the Adam step, into profiles/head_train_adam_bench.json
    python tools/head_train_bench.py --plain --repeats 7       # the plain head (no BatchNorm) beside the BatchNorm head, into profiles/head_plain_bench.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o F35203 -- \
        python tools/head_train_bench.py --features 35203 --steps 50 --no-fit --no-torch --no-dw1 --out DIR/under_profiler.json
                                                       # per-kernel breakdown of ONE width per run (profiles/head_train_kernel_stats_F*.csv)

Per shape (F = 35203 and 19779, H1 = 256, B = 256, drop_rate 0.1): ms per step of the hand-written path and of the same step
written with stock torch ops on the same GPU, each as the median of `--repeats` timed runs of `--steps` back-to-back steps
after a warm-up (HIP events around the run; min / max over the repeats are the spread).  The dW1 + SGD kernel moves at least
X_b + 2 x (W1 + momentum) bytes per step: it is timed alone (relax_head_train_dw1 on the batch the last step left), fused as the
step runs it and unfused (the same tiles writing dW1, then a separate update pass), with bytes / s against that model.  Last: the wall time of one
KoNViD-shaped fit (960 rows, 10 folds, 120 epochs).

--optimizer adam times relax_head_train_step_adam instead (Adam with an L2 term, as fit_head runs it), torch.optim.Adam as the stock
step, and the SGD step of the same state beside them in the same run; the dW1 + Adam kernel moves X_b + 2 x (W1 + both moments)
bytes (252 MB at F = 35203).
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
from relax_vqa_amd import head_train  # noqa: E402
from relax_vqa_amd.engine import RelaxEngine  # noqa: E402

COPY_RATE = 6.29e12   # bytes / s, the measured copy rate the roofline is quoted against


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


def torch_step_fn(F, H1, x, y, rows, optimizer="sgd"):
    import head_train_ref as R
    model = R.Mlp(F, H1, 0.0).cuda()
    drop = torch.nn.Dropout(0.1)
    if optimizer == "adam":
        opt = torch.optim.Adam(model.parameters(), lr=0.001, weight_decay=0.005)
    else:
        opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=0.005)
    model.train()

    def fn():
        xb, yb = x[rows], y[rows]
        opt.zero_grad()
        h = drop(torch.nn.functional.gelu(model.bn1(model.fc1(xb))))
        h = drop(torch.nn.functional.gelu(model.fc2(h)))
        loss = R.mae_rank_loss(model.fc3(h).reshape(-1), yb, 0.6, 1.0)
        loss.backward()
        opt.step()
    return fn


def one_run(fn, steps, warmup):
    """ms per step of `steps` back-to-back calls after a warm-up, between two device events."""
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def spread(samples, steps):
    return {"median_ms": float(np.median(samples)), "min_ms": float(min(samples)), "max_ms": float(max(samples)), "repeats": len(samples),
            "steps": steps}


def torch_plain_step_fn(F, H1, x, y, rows, optimizer):
    import head_plain_ref as P
    model = P.PlainMlp(F, H1, 0.0).cuda()
    drop = torch.nn.Dropout(0.1)
    if optimizer == "adam":
        opt = torch.optim.Adam(model.parameters(), lr=0.001, weight_decay=0.005)
    else:
        opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=0.005)
    model.train()

    def fn():
        xb, yb = x[rows], y[rows]
        opt.zero_grad()
        h = drop(torch.nn.functional.gelu(model.fc1(xb)))
        h = drop(torch.nn.functional.gelu(model.fc2(h)))
        loss = P.mae_rank_loss(model.fc3(h).reshape(-1), yb, 0.6, 1.0)
        loss.backward()
        opt.step()
    return fn


def plain_bench(args, eng):
    """--plain: the plain head's step (no BatchNorm) beside the BatchNorm head's, under SGD and under Adam, and the plain step in stock
    torch ops.  An engine holds one training state, so the two variants alternate state by state: each of the `--repeats` rounds
    builds the plain state, times `--steps` steps, then the same for the BatchNorm state; medians and spread over the rounds."""
    H1, B, n = 256, 256, 960
    res = {"device": torch.cuda.get_device_name(0), "B": B, "H1": H1, "drop_rate": 0.1, "arithmetic": "fp32 (the only one built)",
           "timing": "device events around --steps back-to-back steps after --warmup; median / min / max over --repeats alternated rounds",
           "shapes": {}}
    for F in [int(v) for v in args.features.split(",")]:
        g = torch.Generator(device="cuda").manual_seed(F)
        xp = torch.zeros((n, (F + 31) // 32 * 32), device="cuda")
        xp[:, :F] = torch.rand((n, F), device="cuda", generator=g)
        y = 1 + 4 * torch.rand((n,), device="cuda", generator=g)
        rows = torch.randperm(n, device="cuda", generator=g)[:B].to(torch.int32)
        inits = {bn: head_train.init_state_dict(F, H1, seed=1, batchnorm=bn) for bn in (False, True)}
        entry = {}
        for optimizer in ("sgd", "adam"):
            samples = {False: [], True: []}
            for _ in range(args.repeats):
                for bn in (False, True):
                    tr = head_train.HeadTrainer(eng, F, H1, max_batch=B, batchnorm=bn)
                    tr.import_state(inits[bn])
                    counter = [0]

                    def step():
                        if optimizer == "adam":
                            tr.step_adam(xp, y, rows, 0.001, weight_decay=0.005, drop_rate=0.1, seed=1, step=counter[0])
                        else:
                            tr.step(xp, y, rows, 0.01, 0.9, 0.005, 0.6, 1.0, 0.1, seed=1, step=counter[0])
                        counter[0] += 1
                    samples[bn].append(one_run(step, args.steps, args.warmup))
            entry[f"hip_plain_{optimizer}"] = spread(samples[False], args.steps)
            entry[f"hip_batchnorm_{optimizer}"] = spread(samples[True], args.steps)
            if not args.no_torch:
                fn = torch_plain_step_fn(F, H1, xp[:, :F].contiguous(), y, rows.long(), optimizer)
                entry[f"torch_plain_{optimizer}"] = spread([one_run(fn, args.steps, args.warmup) for _ in range(args.repeats)], args.steps)
                del fn
        res["shapes"][str(F)] = entry
        print(F, json.dumps(entry))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plain", action="store_true", help="the plain head (no BatchNorm) beside the BatchNorm head, SGD and Adam; "
                    "into profiles/head_plain_bench.json")
    ap.add_argument("--optimizer", choices=("sgd", "adam"), default="sgd")
    ap.add_argument("--out", default=None, help="default: profiles/head_train_bench.json, or head_train_adam_bench.json under --optimizer adam")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-fit", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-dw1", action="store_true")
    ap.add_argument("--features", default="35203,19779", help="comma-separated feature widths")
    args = ap.parse_args()
    adam = args.optimizer == "adam"
    if args.plain:
        args.out = args.out or os.path.join(ROOT, "profiles", "head_plain_bench.json")
        return plain_bench(args, RelaxEngine(0))
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "head_train_adam_bench.json" if adam else "head_train_bench.json")
    eng = RelaxEngine(0)
    res = {"optimizer": args.optimizer, "device": torch.cuda.get_device_name(0), "B": 256, "H1": 256, "drop_rate": 0.1, "arithmetic": "fp32 (the only one built)",
           "shapes": {}}
    H1, B, n = 256, 256, 960
    for F in [int(v) for v in args.features.split(",")]:
        g = torch.Generator(device="cuda").manual_seed(F)
        xp = torch.zeros((n, (F + 31) // 32 * 32), device="cuda")
        xp[:, :F] = torch.rand((n, F), device="cuda", generator=g)
        y = 1 + 4 * torch.rand((n,), device="cuda", generator=g)
        rows = torch.randperm(n, device="cuda", generator=g)[:B].to(torch.int32)
        tr = head_train.HeadTrainer(eng, F, H1, max_batch=B)
        tr.import_state(head_train.init_state_dict(F, H1, seed=1))
        counter = [0]

        def hip_step():
            tr.step(xp, y, rows, 0.01, 0.9, 0.005, 0.6, 1.0, 0.1, seed=1, step=counter[0])
            counter[0] += 1

        def hip_step_adam():
            tr.step_adam(xp, y, rows, 0.001, weight_decay=0.005, drop_rate=0.1, seed=1, step=counter[0])
            counter[0] += 1
        fpad = xp.shape[1]
        if adam:
            entry = {"hip": timed(hip_step_adam, args.steps, args.repeats, args.warmup)}
            model_bytes = 4.0 * (B * fpad + 6 * H1 * fpad)
            dw1_only = lambda fused: tr.dw1_adam_only(fused, B, lr=1e-6)
        else:
            entry = {"hip": timed(hip_step, args.steps, args.repeats, args.warmup)}
            model_bytes = 4.0 * (B * fpad + 4 * H1 * fpad)
            dw1_only = lambda fused: tr.dw1_only(fused, B, lr=1e-6)
        entry[f"dw1_{args.optimizer}_model_bytes"] = model_bytes
        entry[f"dw1_{args.optimizer}_roofline_us"] = model_bytes / COPY_RATE * 1e6
        if not args.no_dw1:
            for name, fused in ((f"dw1_{args.optimizer}_fused", True), ("dw1_gemm_then_update_unfused", False)):
                t = timed(lambda: dw1_only(fused), args.steps, args.repeats, args.warmup)
                t["model_bytes_per_s"] = model_bytes / (t["median_ms"] * 1e-3)
                t["frac_of_copy_rate"] = t["model_bytes_per_s"] / COPY_RATE
                entry[name] = t
        if not args.no_torch:
            entry["torch"] = timed(torch_step_fn(F, H1, xp[:, :F].contiguous(), y, rows.long(), args.optimizer), args.steps, args.repeats,
                                   args.warmup)
        if adam:   # the SGD step beside it, from a fresh optimizer on the same state
            tr.import_state(head_train.init_state_dict(F, H1, seed=1))
            entry["hip_sgd"] = timed(hip_step, args.steps, args.repeats, args.warmup)
        res["shapes"][str(F)] = entry
        print(F, json.dumps(entry))
    if not args.no_fit:
        rng = np.random.RandomState(0)
        F = 35203
        del tr, xp
        x = torch.rand((n, F), device="cuda")
        mos = (1 + 4 * rng.uniform(size=n)).astype(np.float32)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cfg = dict(n_splits=10, epochs=120, patience=10 ** 6)   # no early stop: every epoch runs
        if adam:
            cfg.update(optimizer_type="adam", initial_lr=1e-3)
        _, _, hist = eng.fit_head(x, mos, cfg)
        torch.cuda.synchronize()
        res["konvid_shaped_fit"] = {"rows": n, "F": F, "folds": 10, "epochs": 120, "wall_s": time.perf_counter() - t0,
                                    "epochs_run": int(sum(len(v) for v in hist["train_loss"]))}
        print(json.dumps(res["konvid_shaped_fit"]))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
