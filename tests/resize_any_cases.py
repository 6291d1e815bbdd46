"""The cases the any-size resize is tested at (tests/test_resize_any_cpu.py pins the oracle to Pillow at them,
tests/test_gpu_resize_any.py the device to the oracle): seeded random uint8 frames and their oracle resizes, made once."""
import numpy as np

from oracle import resize_ref

# (H, W) -> (out_h, out_w), N
CASES = [
    ((37, 53), (16, 30), 2),      # odd sizes, downscale both ways
    ((37, 53), (37, 20), 2),      # vertical pass skipped
    ((37, 53), (50, 53), 2),      # horizontal pass skipped, upscale
    ((18, 34), (48, 80), 2),      # upscale both ways
    ((33, 60), (33, 60), 2),      # both skipped: a copy
    ((135, 240), (68, 120), 2),   # aligned rows, several workgroups, H % 4 != 0
    ((5, 7), (1, 1), 2),
    ((1, 1), (3, 5), 2),
    ((64, 48), (63, 47), 2),      # scale just above 1
    ((40, 64), (24, 40), 2),      # W * 3 % 16 == 0: the 16-byte path, and the bytewise one from a base one byte off
    ((1080, 1920), (270, 480), 2),   # a real size
    ((3, 8192), (2, 100), 1),     # the widest row: the row stage above 64 KiB of LDS
]
# the 224 entries (relax_resize_frames / relax_resize_residual) on the same kernels: the widest rows they take (H = 5), and the input sizes
# whose -> 224 tables are checked for coefficients inside 24 bits
WIDEST_224 = [5456, 5461]
IN_SIZES_224 = [1, 2, 3, 100, 223, 224, 225, 448, 1080, 1920, 2160, 3840, 5456, 5457, 5461, 8192, 16384]
TABLE_PAIRS = [(53, 30), (37, 16), (34, 80), (18, 48), (240, 120), (1080, 270), (1920, 480), (2160, 224), (7, 1), (1, 5), (64, 63)]

_frames, _refs = {}, {}


def frames(hw, n):
    """uint8 [n, H, W, 3], seeded by the shape; half of the first frame quantised to multiples of 16 (flat runs, as test_gpu_resize.py)"""
    if (hw, n) not in _frames:
        h, w = hw
        f = np.random.default_rng(1000 * h + w).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
        f[0, : h // 2] = f[0, : h // 2] // 16 * 16
        f.setflags(write=False)
        _frames[(hw, n)] = f
    return _frames[(hw, n)]


def reference(hw, out, n, filt):
    """oracle.resize_ref.resize of frames(hw, n): uint8 [n, out_h, out_w, 3]"""
    key = (hw, out, n, filt)
    if key not in _refs:
        r = np.stack([resize_ref.resize(f, out[0], out[1], filt) for f in frames(hw, n)])
        r.setflags(write=False)
        _refs[key] = r
    return _refs[key]
