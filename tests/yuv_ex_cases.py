"""Shared tables of the RELAX_YUVF_* tests (tests/test_yuv_ex_cpu.py, tests/test_gpu_yuv_ex.py): names, ids, sizes, seeds, and the
frame builders.  The expected bytes always come from sampling.yuv_samples + sampling.yuv_frame_bgr_ex, the numpy statement."""
import numpy as np

from relax_vqa_amd import sampling

OLD_NAMES = ["yuv420p", "yuvj420p", "yuv422p", "yuvj422p", "yuv444p", "yuvj444p", "nv12"]
NEW_FORMATS = {                                       # name -> RELAX_YUVF_* id, written out (include/relax_hip.h)
    "nv21": 4, "yuyv422": 5, "uyvy422": 6, "yuv411p": 7, "yuv410p": 8, "yuv420p10le": 9, "yuv422p10le": 10, "yuv444p10le": 11,
    "yuv420p12le": 12, "yuv422p12le": 13, "yuv444p12le": 14, "p010le": 15,
}
NEW_NAMES = list(NEW_FORMATS)
# relax_yuv_format_info's table written out, by format id: sample bytes, depth, shift, hshift, vshift, packing (0 planar, 1 semi-planar,
# 2 packed), swap (semi-planar: V first; packed: chroma first)
FORMAT_INFO = [
    [1, 8, 0, 1, 1, 0, 0],     # 0 420P
    [1, 8, 0, 1, 0, 0, 0],     # 1 422P
    [1, 8, 0, 0, 0, 0, 0],     # 2 444P
    [1, 8, 0, 1, 1, 1, 0],     # 3 NV12
    [1, 8, 0, 1, 1, 1, 1],     # 4 NV21
    [1, 8, 0, 1, 0, 2, 0],     # 5 YUYV422
    [1, 8, 0, 1, 0, 2, 1],     # 6 UYVY422
    [1, 8, 0, 2, 0, 0, 0],     # 7 411P
    [1, 8, 0, 2, 2, 0, 0],     # 8 410P
    [2, 10, 0, 1, 1, 0, 0],    # 9 420P10LE
    [2, 10, 0, 1, 0, 0, 0],    # 10 422P10LE
    [2, 10, 0, 0, 0, 0, 0],    # 11 444P10LE
    [2, 12, 0, 1, 1, 0, 0],    # 12 420P12LE
    [2, 12, 0, 1, 0, 0, 0],    # 13 422P12LE
    [2, 12, 0, 0, 0, 0, 0],    # 14 444P12LE
    [2, 10, 6, 1, 1, 1, 0],    # 15 P010LE
]
REFUSED_NAMES = ["pal8", "yuv420p10be", "yuv420p16le", "gbrp", "yuva420p", "gray", "", "YUV420P"]
TWO_BYTE = [n for n in NEW_NAMES if n.endswith("le")]

# W, H: 1x1 and 2x2, odd sizes, sizes off the 16-pixel lane by one and two, more than one block, the 16-byte path (64x32, 64x36,
# 960x540), 4:1:0's partial row groups (18 = 4*4 + 2, 131 = 4*32 + 3)
CPU_SIZES = [(1, 1), (2, 2), (5, 7), (33, 17), (34, 18), (64, 36)]
GPU_SIZES = [(2, 2), (16, 2), (34, 18), (97, 131), (64, 32), (64, 36), (960, 540)]
SMALL = 97 * 131                                      # every matrix and range up to here: every size but 960x540, which runs BT.601 limited alone
COMBOS = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)]

# frame bytes written out: (W, H) -> name -> bytes
FRAME_BYTES_BY_SIZE = {
    (1, 1): {"nv21": 3, "yuyv422": 4, "uyvy422": 4, "yuv411p": 3, "yuv410p": 3, "yuv420p10le": 6, "yuv422p10le": 6, "yuv444p10le": 6, "yuv420p12le": 6, "yuv422p12le": 6, "yuv444p12le": 6, "p010le": 6, "yuv420p": 3, "yuv422p": 3, "yuv444p": 3, "nv12": 3},
    (2, 2): {"nv21": 6, "yuyv422": 8, "uyvy422": 8, "yuv411p": 8, "yuv410p": 6, "yuv420p10le": 12, "yuv422p10le": 16, "yuv444p10le": 24, "yuv420p12le": 12, "yuv422p12le": 16, "yuv444p12le": 24, "p010le": 12, "yuv420p": 6, "yuv422p": 8, "yuv444p": 12, "nv12": 6},
    (5, 7): {"nv21": 59, "yuyv422": 84, "uyvy422": 84, "yuv411p": 63, "yuv410p": 43, "yuv420p10le": 118, "yuv422p10le": 154, "yuv444p10le": 210, "yuv420p12le": 118, "yuv422p12le": 154, "yuv444p12le": 210, "p010le": 118, "yuv420p": 59, "yuv422p": 77, "yuv444p": 105, "nv12": 59},
    (33, 17): {"nv21": 867, "yuyv422": 1156, "uyvy422": 1156, "yuv411p": 867, "yuv410p": 651, "yuv420p10le": 1734, "yuv422p10le": 2278, "yuv444p10le": 3366, "yuv420p12le": 1734, "yuv422p12le": 2278, "yuv444p12le": 3366, "p010le": 1734, "yuv420p": 867, "yuv422p": 1139, "yuv444p": 1683, "nv12": 867},
    (34, 18): {"nv21": 918, "yuyv422": 1224, "uyvy422": 1224, "yuv411p": 936, "yuv410p": 702, "yuv420p10le": 1836, "yuv422p10le": 2448, "yuv444p10le": 3672, "yuv420p12le": 1836, "yuv422p12le": 2448, "yuv444p12le": 3672, "p010le": 1836, "yuv420p": 918, "yuv422p": 1224, "yuv444p": 1836, "nv12": 918},
    (64, 36): {"nv21": 3456, "yuyv422": 4608, "uyvy422": 4608, "yuv411p": 3456, "yuv410p": 2592, "yuv420p10le": 6912, "yuv422p10le": 9216, "yuv444p10le": 13824, "yuv420p12le": 6912, "yuv422p12le": 9216, "yuv444p12le": 13824, "p010le": 6912, "yuv420p": 3456, "yuv422p": 4608, "yuv444p": 6912, "nv12": 3456},
}
FRAME_BYTES = {(name, W, H): v for (W, H), row in FRAME_BYTES_BY_SIZE.items() for name, v in row.items()}


def fmt(name):
    return sampling.yuv_format(name)


def frame_bytes(name, H, W):
    return sampling.yuv_frame_bytes_ex(fmt(name)[0], H, W)


def random_frames(name, H, W, n, seed):
    """n frames of random BYTES: 2-byte samples then carry garbage above a 10 / 12-bit value and below a P010 value."""
    return np.random.default_rng(seed).integers(0, 256, (n, frame_bytes(name, H, W)), dtype=np.uint8)


def host_bgr(frame, name, H, W, matrix="bt601", full_range=None):
    f, full = fmt(name)
    y, u, v, depth = sampling.yuv_samples(frame, f, H, W)
    return sampling.yuv_frame_bgr_ex(y, u, v, depth, matrix=matrix, full_range=full if full_range is None else full_range)


def pack_frame(name, y, u, v, filler=0):
    """Y [H,W], U and V [ch,cw] at native depth -> the frame's bytes (padding bytes and unused bits = filler's)."""
    f, _ = fmt(name)
    H, W = y.shape
    t, p = sampling.yuv_format_info(f), sampling.yuv_plan_ex(f, H, W)
    frame = np.full(p["frame_bytes"], filler, np.uint8)

    def put(plane, off, stride, step):
        rows, cols = plane.shape
        at = off + np.arange(rows, dtype=np.int64)[:, None] * stride + np.arange(cols, dtype=np.int64)[None, :] * step
        word = plane.astype(np.int64) << t["shift"]
        frame[at] = word & 255
        if t["sample_bytes"] == 2:
            frame[at + 1] = word >> 8
    put(np.asarray(y), p["y_off"], p["y_stride"], p["y_step"])
    put(np.asarray(u), p["u_off"], p["c_stride"], p["c_step"])
    put(np.asarray(v), p["v_off"], p["c_stride"], p["c_step"])
    return frame


def grey_frame(name, H, W, seed):
    """Random luma under neutral chroma (128 << (depth - 8))."""
    f, _ = fmt(name)
    t, p = sampling.yuv_format_info(f), sampling.yuv_plan_ex(f, H, W)
    rng = np.random.default_rng(seed)
    c = np.full((p["ch"], p["cw"]), 128 << (t["depth"] - 8))
    return pack_frame(name, rng.integers(0, 1 << t["depth"], (H, W)), c, c)


def records(bgr):
    """[N,H,W,3] -> the greyscale records (tests/greyscale_cases.py's statement of the rule)."""
    from tests import greyscale_cases
    return greyscale_cases.records(bgr)


def threshold_frames(name, H, W, seed, matrix="bt601", full_range=False):
    """(the last grey frame, the first colour frame): a grey frame whose one V sample is raised one code value at a time until the
    largest absolute difference passes the threshold of 3, and the frame one code value before."""
    from tests import greyscale_cases
    f, _ = fmt(name)
    t, p = sampling.yuv_format_info(f), sampling.yuv_plan_ex(f, H, W)
    s = t["depth"] - 8
    rng = np.random.default_rng(seed)
    y = np.full((H, W), 120 << s)
    y[rng.integers(0, H), rng.integers(0, W)] = 121 << s
    c = np.full((p["ch"], p["cw"]), 128 << s)
    before = pack_frame(name, y, c, c)
    for delta in range(1, 64 << s):
        v = c.copy()
        v[p["ch"] // 2, p["cw"] // 2] += delta
        frame = pack_frame(name, y, c, v)
        rec = greyscale_cases.records(host_bgr(frame, name, H, W, matrix, full_range)[None])
        if not greyscale_cases.is_greyscale(rec, mode="abs")[0]:
            return before, frame
        before = frame
    raise AssertionError("no chroma step crossed the threshold")
