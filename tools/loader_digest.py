#!/usr/bin/env python3
"""What the model loaders put on the device, seen through what the forwards compute from it (GPU box only).
  python tools/loader_digest.py digest [OUT.json]     sha256 of every output tensor of the matrix below
  python tools/loader_digest.py load [ROUNDS]         wall-clock seconds of load_resnet50 + load_vgg16 + load_vit("vit_base") incl. the final
                                                      synchronise, per round on a fresh engine, and device_bytes_held: hipMemGetInfo's free bytes
                                                      before the engine exists minus after the loads (the three models + the handle's own allocations)
RELAX_HIP_LIB selects the build: run once per build and compare - two builds whose loaders derive the same weights print the same digests.
Matrix (synthetic state dicts of synth.py, N = 3 fragments of synth.synthetic_clip, gemm_split_k 0): ResNet-50 layer stack + pool + all 15
taps under gemm_precision 0 / 1 / 2 / 3 and, under 3, with each of rn_h2, rn_h2_early, rn_fuse, rn_c1_h2, x6_fp32_rows off in turn; VGG-16
layer stack + pool + taps 0, 12, 13, 14 under 0 / 2 / 3; ViT-B/16, ViT-B/8 and vit_tiny (dim 192: bf16x6 under 3) tokens + pooled + CLS
attention under 0 / 2 / 3 and, under 3, with att_h2 off."""
import hashlib
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import relax_vqa_amd  # noqa: E402,F401
from relax_vqa_amd import synth  # noqa: E402
from relax_vqa_amd.engine import RelaxEngine  # noqa: E402

RN_SWITCHES = ("rn_h2", "rn_h2_early", "rn_fuse", "rn_c1_h2", "x6_fp32_rows")


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def settings(switches, precisions):
    """(label, options) of one model's runs: every precision, then precision 3 with each switch off alone"""
    runs = [(f"p{p}", {"gemm_precision": p}) for p in precisions]
    return runs + [(f"p3 {s}=0", {"gemm_precision": 3, s: 0}) for s in switches]


def with_options(eng, opts, switches):
    for s in switches:
        eng.set_option(s, 1)
    for k, v in opts.items():
        eng.set_option(k, v)


def digest():
    eng = RelaxEngine(0)
    eng.set_option("gemm_split_k", 0)
    fr = eng.fragment_pairs(torch.from_numpy(synth.synthetic_clip(2, 240, 320, clip_id=5)).cuda())
    frags = torch.cat([fr["ori_frag"], fr["diff_frag"]])[:3].contiguous()
    out = {}
    eng.load_resnet50(synth.resnet50_state_dict())
    for label, opts in settings(RN_SWITCHES, (0, 1, 2, 3)):
        with_options(eng, opts, RN_SWITCHES)
        ls, pool, taps = eng.resnet50_features(frags, taps=range(15))
        out[f"resnet50 {label} layer_stack"], out[f"resnet50 {label} pool"] = sha(ls), sha(pool)
        out.update({f"resnet50 {label} tap{i}": sha(taps[i]) for i in range(15)})
    with_options(eng, {"gemm_precision": 3}, RN_SWITCHES)
    eng.load_vgg16(synth.vgg16_state_dict())
    for label, opts in settings((), (0, 2, 3)):
        with_options(eng, opts, ())
        ls, pool, taps = eng.vgg16_features(frags, taps=(0, 12, 13, 14))
        out[f"vgg16 {label} layer_stack"], out[f"vgg16 {label} pool"] = sha(ls), sha(pool)
        out.update({f"vgg16 {label} tap{i}": sha(t) for i, t in taps.items()})
    for name, patch in (("vit_base", 16), ("vit_base", 8), ("vit_tiny", 16)):
        eng.load_vit(synth.vit_state_dict(name, patch=patch), name)
        for label, opts in settings(("att_h2",), (0, 2, 3)):
            with_options(eng, opts, ("att_h2",))
            tokens, pooled, att = eng.vit_features(frags, tokens=True, attention=True)
            for what, t in (("tokens", tokens), ("pooled", pooled), ("cls_attention", att)):
                out[f"{name}/{patch} {label} {what}"] = sha(t)
    torch.cuda.synchronize()
    return out


def load_rounds(rounds):
    sds = synth.resnet50_state_dict(), synth.vgg16_state_dict(), synth.vit_state_dict("vit_base")
    res = []
    for r in range(rounds):
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        eng = RelaxEngine(0)
        t0 = time.perf_counter()
        eng.load_resnet50(sds[0])
        eng.load_vgg16(sds[1])
        eng.load_vit(sds[2], "vit_base")
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res.append({"round": r, "load_s": round(dt, 4), "device_bytes_held": free0 - torch.cuda.mem_get_info()[0]})
        eng.close()
    return res


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "digest"
    if mode == "load":
        result = {"lib": os.environ.get("RELAX_HIP_LIB", "in-tree"), "rounds": load_rounds(int(sys.argv[2]) if len(sys.argv) > 2 else 3)}
    else:
        result = {"lib": os.environ.get("RELAX_HIP_LIB", "in-tree"), "digests": digest()}
    print(json.dumps(result))
    if mode == "digest" and len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(result, f, indent=1)
