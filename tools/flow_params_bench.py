"""Times relax_optical_flow_ex under parameter sets other than the reference's literals, against the literal set in the same run, and
writes profiles/flow_params_bench.json.  Device events, median of --reps runs, --pairs pairs per call, flow image only (what the
pipeline asks for).  Per resolution:
  literal_old / literal_ex   relax_optical_flow and relax_optical_flow_ex at the literals, alternated: the same launches
  every other set            ms per pair, and GB/s on the algorithmic bytes flow_chunk tallies (relax_profile_read kind 6, read in an
                             extra profiled call that is not timed)
  fused / two_kernel         winsize 15 sets: flow_fused 1 against 0 (flow_iteration | update_matrices_k + box_solve_fused)
Usage: python tools/flow_params_bench.py [--sizes 540x960,1080x1920,2160x3840] [--pairs 32] [--reps 7] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LITERAL = dict(pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2)
SETS = {
    "winsize9": dict(winsize=9), "winsize25": dict(winsize=25), "winsize33": dict(winsize=33), "winsize63": dict(winsize=63),
    "poly_n7": dict(poly_n=7, poly_sigma=1.5), "iterations1": dict(iterations=1), "iterations5": dict(iterations=5),
    "pyr_scale0.8": dict(pyr_scale=0.8, levels=4),
}
DEEP = {"levels4": dict(levels=4), "levels5": dict(levels=5)}     # 2160p only: the motivating case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="540x960,1080x1920,2160x3840")
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_params_bench.json"))
    args = ap.parse_args()
    import torch
    import relax_vqa_amd  # noqa: F401
    from relax_vqa_amd import synth
    from relax_vqa_amd.engine import RelaxEngine

    eng = RelaxEngine(0)

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

    def stage_bytes(fn):
        eng.profile_enable(True)
        try:
            fn()
            torch.cuda.synchronize()
            return eng.profile_read(6)[1]
        finally:
            eng.profile_enable(False)

    def row(times, nbytes):
        ms = statistics.median(times)
        return {"ms_per_pair": ms / args.pairs, "spread_ms_per_pair": (max(times) - min(times)) / args.pairs,
                "algorithmic_gb": nbytes / 1e9, "gb_per_s": nbytes / 1e9 / (ms / 1e3)}

    out = {"device": torch.cuda.get_device_name(0), "pairs": args.pairs, "reps": args.reps, "timing": "device events, median",
           "sizes": {}}
    for size in args.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        distinct = torch.from_numpy(synth.synthetic_clip(min(args.pairs, 4), H, W, 1)).cuda()      # (four distinct pairs, repeated: the host makes them slowly)
        clip = distinct.repeat((args.pairs + 3) // 4, 1, 1, 1, 1)[:args.pairs].contiguous()
        res = {}
        old = lambda: eng.optical_flow(clip)                                   # noqa: E731
        new = lambda: eng.optical_flow_ex(clip, **LITERAL)                     # noqa: E731
        t_old, t_new = [], []
        for _ in range(2):                                                     # alternated in the same process
            t_old += timed(old)
            t_new += timed(new)
        nb = stage_bytes(old)
        res["literal_old"], res["literal_ex"] = row(t_old, nb), row(t_new, stage_bytes(new))
        sets = dict(SETS, **(DEEP if H >= 2160 else {}))
        for name, change in sets.items():
            params = {**LITERAL, **change}
            fn = lambda: eng.optical_flow_ex(clip, **params)                   # noqa: E731
            res[name] = dict(row(timed(fn), stage_bytes(fn)), params=params)
            if params["winsize"] == 15:                                        # both iteration paths exist
                eng.set_option("flow_fused", 0)
                try:
                    res[name]["two_kernel"] = row(timed(fn), stage_bytes(fn))
                finally:
                    eng.set_option("flow_fused", 1)
            res[name]["vs_literal"] = res[name]["ms_per_pair"] / res["literal_old"]["ms_per_pair"]
            print(size, name, json.dumps(res[name]), flush=True)
        print(size, "literal", json.dumps({k: res[k] for k in ("literal_old", "literal_ex")}), flush=True)
        out["sizes"][size] = res
        del clip
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:                                         # (rewritten after every size: a long run leaves what it has)
            json.dump(out, f, indent=1)
            f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
