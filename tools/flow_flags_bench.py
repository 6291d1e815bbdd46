"""Times relax_optical_flow_flags' two modes and writes profiles/flow_flags_bench.json.  Device events, median of --reps runs with min and
max, --pairs pairs per call, flow image only (what the pipeline asks for), one card, one session.  Per resolution:
  gauss_winN / box_winN   flags 256 and flags 0 at winsize N (the other five parameters the literals), alternated twice in the same run
  init_literal            the literal set with flags 4 (a smooth field) beside the literal set with flags 0
  resize_area             relax_flow_initial_level alone on the same field (the area resize to the coarsest level, its table upload and wait)
--trace-one WINSIZE runs ONE flags-256 call at that window and the first size and nothing else: the program of a kernel trace taken in a run of
its own, from which gauss_solve_any's share of the stage is read.
Usage: python tools/flow_flags_bench.py [--sizes 1080x1920,2160x3840] [--pairs 32] [--reps 7] [--out FILE] [--trace-one WINSIZE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOWS = (9, 15, 33, 63)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1080x1920,2160x3840")
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_flags_bench.json"))
    ap.add_argument("--trace-one", type=int, default=0)
    args = ap.parse_args()
    import numpy as np
    import torch
    import relax_vqa_amd  # noqa: F401
    from relax_vqa_amd import synth
    from relax_vqa_amd.engine import RelaxEngine

    eng = RelaxEngine(0)

    def clip_of(H, W):
        distinct = torch.from_numpy(synth.synthetic_clip(min(args.pairs, 4), H, W, 1)).cuda()      # (four distinct pairs, repeated)
        return distinct.repeat((args.pairs + 3) // 4, 1, 1, 1, 1)[:args.pairs].contiguous()

    if args.trace_one:
        H, W = (int(v) for v in args.sizes.split(",")[0].split("x"))
        clip = clip_of(H, W)
        for _ in range(2):
            eng.optical_flow_flags(clip, winsize=args.trace_one, flags=256)
        torch.cuda.synchronize()
        print("traced", H, W, args.trace_one)
        return

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        return times

    def row(times):
        return {"ms_per_pair": statistics.median(times) / args.pairs, "min": min(times) / args.pairs, "max": max(times) / args.pairs, "samples": len(times)}

    out = {"device": torch.cuda.get_device_name(0), "pairs": args.pairs, "reps": args.reps,
           "timing": "device events around one call; median, min and max over the samples, ms per pair", "sizes": {}}
    for size in args.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        clip = clip_of(H, W)
        res = {}
        for ws in WINDOWS:
            gauss = lambda: eng.optical_flow_flags(clip, winsize=ws, flags=256)      # noqa: E731
            box = lambda: eng.optical_flow_flags(clip, winsize=ws, flags=0)          # noqa: E731
            t_g, t_b = [], []
            for _ in range(2):                                                       # alternated in the same process
                t_g += timed(gauss)
                t_b += timed(box)
            res[f"gauss_win{ws}"], res[f"box_win{ws}"] = row(t_g), row(t_b)
            res[f"gauss_win{ws}"]["vs_box"] = res[f"gauss_win{ws}"]["ms_per_pair"] / res[f"box_win{ws}"]["ms_per_pair"]
            print(size, ws, json.dumps({k: res[k] for k in (f"gauss_win{ws}", f"box_win{ws}")}), flush=True)
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        field = np.stack([3 + 0.75 * np.sin(xx / W * 9 + yy / H * 3), -2 + 0.75 * np.cos(xx / W * 6 - yy / H * 8)], axis=-1)
        init = torch.from_numpy(field).cuda()[None].repeat(args.pairs, 1, 1, 1).contiguous()
        with_init = lambda: eng.optical_flow_flags(clip, flags=4, initial_flow=init)     # noqa: E731
        literal = lambda: eng.optical_flow_flags(clip, flags=0)                          # noqa: E731
        level = lambda: eng.flow_initial_level(init)                                     # noqa: E731
        t_i, t_l = [], []
        for _ in range(2):
            t_i += timed(with_init)
            t_l += timed(literal)
        res["init_literal"], res["literal"], res["resize_area"] = row(t_i), row(t_l), row(timed(level))
        print(size, json.dumps({k: res[k] for k in ("init_literal", "literal", "resize_area")}), flush=True)
        out["sizes"][size] = res
        del clip, init
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:                                         # (rewritten after every size: a long run leaves what it has)
            json.dump(out, f, indent=1)
            f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
