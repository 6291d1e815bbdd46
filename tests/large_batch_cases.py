"""The cases of tests/test_gpu_large_batch.py: which tensor each one pushes past 2^31 or 2^32 bytes, at which count, and the periodic
construction that makes a multi-GB result checkable (helper of that file and of tests/test_large_batch_cases_cpu.py; pure Python, torch
is imported inside the functions that compare tensors).

The headline benchmark hands 2048 fragments to each backbone in one call; activation tensors cross 2^31 and 2^32 bytes between 512 and
2048 images, and the kernels have arms that only run there: descriptor sizes clamped at 2^31 - 16, 64-bit descriptor bases beside 32-bit
lane offsets, per-image descriptor bases, arena offsets past 4 GiB.  A case takes the SMALLEST count at which its tensor crosses (never
more than the benchmark launches every day: CEILINGS).

Periodic construction: a big input is `small[idx(i)]`, row (or image) i a copy of row i % period of a small block, gathered on the
device.  Every entry point under test computes a row from that row's (image's) input alone when the tail split is off, so row i of the
big result has to be the bits of row i % period of the block's result - that comparison needs no big reference, and the block alone goes
to the fp64 CPU reference.  The period is a prime, so it divides no tile size (64, 128, 256, 512) and no power of two: tiles straddle
period boundaries, and an address that wraps by 2^31 or 2^32 bytes never lands on a row of equal content (wrap_lands_on_equal_content)."""
import ctypes as C
import os
import subprocess

from tests import vit_plan_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WRAPS = (2 ** 31, 2 ** 32)
# nothing here launches more than bench.py does at its default workload: 2048 fragments per backbone ("model": images), 2048 * 197 =
# 403 456 token rows in a GEMM or the 197-token attention ("operator": rows); the operators addressed by image - convolutions, pooling,
# the 785-token attention - are held to the 2048 images ("images": their pixel rows are per image what the benchmark's are, and the
# benchmark runs no 785-token attention whose rows could be the measure: that case stays below the headline's qkv bytes and images)
CEILINGS = {"model": 2048, "operator": 2048 * 197, "images": 2048}
TILE_SIZES = (64, 128, 256, 512)
PERIOD_ROWS = 997          # operator cases addressed by row
PERIOD_IMAGES = 61         # model cases
PERIOD_OP_IMAGES = 7       # operator cases addressed by image (attention, convolutions, pooling): the fp64 reference of the block stays small

# ResNet-50's activation sizes are not exported by the host library (kBig and its neighbours in csrc/resnet50.hip are internal): they are
# restated here from the geometry - conv1 leaves 112 x 112 x 64 values per image, the block outputs of layer1 56 x 56 x 256 (the same count)
RN_CONV1_FLOATS = 112 * 112 * 64
RN_LAYER1_FLOATS = 56 * 56 * 256


def idx(i, period):
    """The index map of the periodic construction: row (image) i of a big tensor is row i % period of the block"""
    return i % period


def host_library(directory):
    """csrc/host_logic.cpp alone with its test entry points (plain g++, no HIP), built into `directory`"""
    out = os.path.join(str(directory), "libhost_large_batch.so")
    src = os.path.join(ROOT, "relax-vqa_amd", "csrc", "host_logic.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-DRELAX_HOST_TEST_API", src, "-o", out], check=True)
    return C.CDLL(out)


def vit_layout(lib, dim, patch):
    """The ViT's per-image sizes from the host library's own exports: the geometry (relax_host_vit_geometry) and the arena totals of the
    two layouts (relax_host_vit_arena_floats), itemised by the slots of host::vit_plan (relax_host_vit_plan: the fp32 layout under
    gemm_precision 0, the plane layout under 2).  The plan's totals are checked against the exported totals: a layout change moves a case
    or fails here."""
    geo = (C.c_int * 5)()
    err = C.create_string_buffer(256)
    if lib.relax_host_vit_geometry(patch, geo, err, 256) != 0:
        raise RuntimeError(err.value.decode())
    _, _, npatch, ntok, patch_k = list(geo)
    totals = (C.c_int64 * 2)()
    lib.relax_host_vit_arena_floats(dim, ntok, npatch, patch_k, totals)
    fp32, planes = (vit_plan_cases.plan(lib, precision=p, dim=dim, patch=patch, patch_k=patch_k, ntok=ntok, npatch=npatch) for p in (0, 2))
    if [fp32["floats"], planes["floats"]] != list(totals):
        raise AssertionError(f"the ViT arena layout moved: {list(totals)} floats per image, the plan's slots end at {[fp32['floats'], planes['floats']]}")
    fp32, planes = vit_plan_cases.slot_sizes(fp32), vit_plan_cases.slot_sizes(planes)
    if fp32["qkv"] != planes["qkv"]:
        raise AssertionError(f"qkv takes {fp32['qkv']} floats per image under fp32 and {planes['qkv']} in the plane layout")
    return {"ntok": ntok, "dim": dim, "arena_fp32": totals[0] * 4, "arena_planes": totals[1] * 4,
            "qkv": fp32["qkv"] * 4,              # fp32 values, or two fp16 planes of as many values
            "hidden": fp32["hidden"] * 4,        # the fc1 output / fc2 input, fp32 or f16x2 planes
            "hidden_x6": planes["hidden"] * 4,   # the same as three bf16 planes of 4 x dim values = the layout's 6 x ntok x dim floats
            "qkv_row": fp32["qkv"] // ntok * 4, "hidden_row": fp32["hidden"] // ntok * 4}


def cases(vit):
    """The case table.  vit: vit_layout(lib, 768, 16) (ViT-B/16).  One entry per (GPU case, tensor it is meant to push past a threshold):
    unit_bytes per `unit` (a row or an image), the threshold, the chosen count, and `slack`: the count reduced by it must be BELOW the
    threshold (16 units of ragged-tile slack, unless the unit of choice is coarser).  level: which of CEILINGS holds ("operator": rows,
    "images" and "model": count); rows = the token / pixel rows the launch has."""
    rn = RN_CONV1_FLOATS * 4
    t = []

    def add(case, tensor, unit, unit_bytes, threshold, count, level, rows, period, slack=16, primary=True):
        t.append(dict(case=case, tensor=tensor, unit=unit, unit_bytes=unit_bytes, threshold=threshold, count=count, level=level, rows=rows,
                      period=period, slack=slack, primary=primary))

    M = GEMM_ROWS
    add("gemm_a", "A [M, 3072] fp32 (fc2's input)", "row", vit["hidden_row"], 2 ** 32, M, "operator", M, PERIOD_ROWS)
    add("gemm_out", "out [M, 3072] fp32 (fc1's output)", "row", vit["hidden_row"], 2 ** 32, M, "operator", M, PERIOD_ROWS)
    n = CONV_IMAGES
    add("conv1x1", "input [n, 56, 56, 256] fp32, addressed by pixel", "image", RN_LAYER1_FLOATS * 4, 2 ** 32, n, "images", n * 56 * 56, PERIOD_OP_IMAGES)
    add("conv3x3", "input [n, 112, 112, 64] fp32 / its planes, addressed by pixel", "image", rn, 2 ** 32, n, "images", n * 112 * 112, PERIOD_OP_IMAGES)
    add("bn_relu_maxpool", "input [n, 112, 112, 64] fp32", "image", rn, 2 ** 32, n, "images", n * 112 * 112, PERIOD_OP_IMAGES)
    add("gap", "input [n, 12544, 64] fp32", "image", rn, 2 ** 32, n, "images", n * 112 * 112, PERIOD_OP_IMAGES)
    # this case was specified at 1201 images (a prime: 14 412 items, about 56 per persistent workgroup); the smallest crossing count is
    # 1183, 18 below it, so its slack is 19 and not 16
    n = ATT_IMAGES
    add("attention", "qkv [n * 197, 2304] fp32", "image", vit["qkv"], 2 ** 31, n, "operator", n * vit["ntok"], PERIOD_OP_IMAGES, slack=19)
    n = ATT_EX_IMAGES
    add("attention_ex", "qkv [n * 785, 576] fp32", "image", ATT_EX_TOKENS * ATT_EX_HEADS * 3 * 64 * 4, 2 ** 31, n, "images", n * ATT_EX_TOKENS,
        PERIOD_OP_IMAGES)
    n = VIT_IMAGES
    add("vit_features", "the fc1 output, fp32 or f16x2 planes", "image", vit["hidden"], 2 ** 32, n, "model", n * vit["ntok"], PERIOD_IMAGES)
    add("vit_features", "the fc1 output as bf16x6 planes", "image", vit["hidden_x6"], 2 ** 32, n, "model", n * vit["ntok"], PERIOD_IMAGES, primary=False)
    add("vit_features", "qkv, fp32 or f16x2 planes", "image", vit["qkv"], 2 ** 31, n, "model", n * vit["ntok"], PERIOD_IMAGES, primary=False)
    add("vit_features", "the arena tensors behind the first (offset from the arena base)", "image", vit["arena_fp32"], 2 ** 32, n, "model",
        n * vit["ntok"], PERIOD_IMAGES, primary=False)
    add("vit_intermediate_layers", "the fc1 output as f16x2 planes (the residual stream lies behind it in the arena)", "image", vit["hidden"], 2 ** 32,
        n, "model", n * vit["ntok"], PERIOD_IMAGES)
    n = RN_IMAGES
    add("resnet50_clip_features", "conv1's raw output / a layer1 block output, fp32", "image", rn, 2 ** 32, n, "model", n * 112 * 112, PERIOD_IMAGES)
    add("resnet50_clip_features", "the same as bf16x6 planes", "image", rn * 3 // 2, 2 ** 32, n, "model", n * 112 * 112, PERIOD_IMAGES, primary=False)
    # whole clips of 32 pairs = 64 fragments: the unit in which this count can be chosen
    n = CLIPS * 2 * CLIP_PAIRS
    add("clip_vectors", "the ViT's fc1 output as f16x2 planes", "image", vit["hidden"], 2 ** 32, n, "model", n * vit["ntok"], CLIP_DISTINCT,
        slack=2 * CLIP_PAIRS)
    add("clip_vectors", "ResNet-50's conv1 output", "image", rn, 2 ** 32, n, "model", n * 112 * 112, CLIP_DISTINCT, slack=2 * CLIP_PAIRS, primary=False)
    return t


GEMM_ROWS = 349531          # >= ceil(2^32 / 12288) = 349526, a ragged last tile at every tile height
GEMM_WIDE, GEMM_NARROW = 3072, 256
CONV_IMAGES = 1341
ATT_IMAGES, ATT_HEADS = 1201, 12
ATT_EX_IMAGES, ATT_EX_TOKENS, ATT_EX_HEADS = 1188, 785, 3
VIT_IMAGES = 1777           # a prime: 350 069 token rows, ragged
RN_IMAGES = 1342            # 2 n of resnet50_clip_features(both, n)
CLIPS, CLIP_PAIRS, CLIP_DISTINCT, CLIP_H, CLIP_W = 28, 32, 3, 270, 480


def wrap_lands_on_equal_content(unit_bytes, period, wrap):
    """Would an address that is off by `wrap` bytes read (or write) a unit of the same content?  Only if the wrap is a whole number of
    periods.  Where it is a whole number of units this is `wrap / unit_bytes mod period == 0`; where it is not, the wrapped address lies
    inside a unit and the content differs anyway."""
    return wrap % (unit_bytes * period) == 0


def _bits(t):
    import torch
    t = t.reshape(t.shape[0], -1)
    if t.dtype in (torch.float32, torch.int32):
        return t.view(torch.int32)
    if t.dtype in (torch.float64, torch.int64):
        return t.view(torch.int64)
    raise TypeError(f"rows_equal_periodic: {t.dtype}")


def _slices(rows, row_bytes, slice_bytes):
    step = max(1, slice_bytes // max(1, row_bytes))
    for lo in range(0, rows, step):
        yield lo, min(rows, lo + step)


def rows_equal_periodic(big, small, period, first=0, slice_bytes=64 << 20):
    """Is row i of `big` the bits of small[idx(first + i)] for every i?  -> None, or the first difference (row, column, got, want); rows
    are the leading dimension, columns the rest flattened.  Works slice by slice (at most slice_bytes of `big` and as much of expanded
    `small` at a time) on the device the tensors are on; only the one differing pair of values ever reaches the host."""
    import torch
    if big.shape[1:] != small.shape[1:] or small.shape[0] < min(period, first + big.shape[0]) or big.dtype != small.dtype:
        raise ValueError(f"rows_equal_periodic: big {tuple(big.shape)} {big.dtype}, small {tuple(small.shape)} {small.dtype}, period {period}")
    b, s = _bits(big), _bits(small)
    for lo, hi in _slices(b.shape[0], b.shape[1] * b.element_size(), slice_bytes):
        want = s[idx(torch.arange(first + lo, first + hi, device=b.device), period)]
        ne = b[lo:hi] != want
        if bool(ne.any()):
            flat = int(ne.reshape(-1).to(torch.uint8).argmax())
            r, c = divmod(flat, b.shape[1])
            return (lo + r, c, big.reshape(big.shape[0], -1)[lo + r, c].item(), small.reshape(small.shape[0], -1)[idx(first + lo + r, period), c].item())
    return None


def rows_close_periodic(big, small, period, rtol, atol_frac, first=0, slice_bytes=64 << 20):
    """gpu_common.assert_close(big, small expanded by the index map, rtol, atol_frac) without the expanded tensor or a host copy:
    |got - want| <= rtol |want| + atol_frac x mean |want|, the mean over the expanded tensor.  -> (worst err / bound, row, column)."""
    import torch
    b, s = big.reshape(big.shape[0], -1), small.reshape(small.shape[0], -1).double()
    n = b.shape[0]
    rows = torch.arange(first, first + n, device=b.device)
    times = torch.bincount(idx(rows, period), minlength=s.shape[0]).double()          # how often each block row occurs in the expansion
    floor = atol_frac * (float((s.abs().sum(dim=1) * times).sum()) / (n * b.shape[1]) + 1e-30)
    worst = (0.0, -1, -1)
    for lo, hi in _slices(n, b.shape[1] * 8, slice_bytes):
        want = s[idx(rows[lo:hi], period)]
        got = b[lo:hi].double()
        if not bool(torch.isfinite(got).all()):
            return (float("inf"), lo, -1)
        ratio = (got - want).abs() / (rtol * want.abs() + floor)
        flat = int(ratio.reshape(-1).argmax())
        r, c = divmod(flat, b.shape[1])
        if float(ratio[r, c]) > worst[0]:
            worst = (float(ratio[r, c]), lo + r, c)
    return worst
