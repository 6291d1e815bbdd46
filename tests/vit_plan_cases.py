"""host::vit_plan (csrc/host_logic.cpp) through its test export: the call, the rule of every route field restated from the plan's own
description, and the slot sizes of an arena layout (helper of tests/test_vit_plan_cpu.py, tests/test_gpu_vit_plan.py and
tests/large_batch_cases.py; pure Python)."""
import ctypes as C

F32, X6, H2 = 0, 1, 2                                                     # VitArith
ATTENTION = ("attention", "attention_stream_f32", "attention_x6", "attention_stream_x6", "attention_h2", "attention_stream_h2")   # VitAttention
ROUTES = ("arith", "patch_embed", "qkv_planes", "attention", "attention_only", "final_norm")
SLOTS = ("patches", "embedded", "residual", "operand", "qkv", "final", "hidden")    # by role; `floats` (the total) follows them


def plan(lib, precision=3, att_h2=1, att_h2_stream=1, dim=768, depth=12, heads=12, patch=16, patch_k=768, ntok=197, npatch=196,
         tokens=0, pooled=1, cls_attention=0, n_last=0):
    """relax_host_vit_plan -> dict of the route fields (attention by name), the slot offsets and `floats`, in floats per image"""
    args = (C.c_int * 14)(precision, att_h2, att_h2_stream, dim, depth, heads, patch, patch_k, ntok, npatch, tokens, pooled, cls_attention, n_last)
    out = (C.c_int64 * 14)()
    lib.relax_host_vit_plan(args, out)
    p = dict(zip(ROUTES + SLOTS + ("floats",), out))
    p["attention"] = ATTENTION[p["attention"]]
    return p


def expected_routes(precision, att_h2, att_h2_stream, dim, patch, ntok, tokens, pooled, cls_attention, n_last):
    """The rules, one line each"""
    arith = H2 if precision == 3 and dim % 256 == 0 else X6 if precision >= 2 else F32
    qkv_planes = arith == H2 and bool(att_h2) and (ntok == 197 or bool(att_h2_stream))
    family = "h2" if qkv_planes else "f32" if arith == F32 else "x6"
    single = {"f32": "attention", "x6": "attention_x6", "h2": "attention_h2"}
    attention_only = bool(cls_attention) and not tokens and not pooled
    return {"arith": arith,
            "patch_embed": X6 if arith == H2 and patch == 8 else arith,
            "qkv_planes": int(qkv_planes),
            "attention": single[family] if ntok == 197 else "attention_stream_" + family,
            "attention_only": int(attention_only),
            "final_norm": int(n_last == 0 and not attention_only)}


def slot_sizes(p):
    """floats per image of every slot of a plan: up to the next offset in carving order.  `final` is the one declared alias: under fp32 it is
    the operand slot again and has no extent of its own (its offset equals operand's)"""
    order = sorted((s for s in SLOTS if not (s == "final" and p["final"] == p["operand"])), key=lambda s: p[s])
    ends = [p[s] for s in order[1:]] + [p["floats"]]
    sizes = {s: e - p[s] for s, e in zip(order, ends)}
    sizes.setdefault("final", sizes["operand"])
    return sizes
