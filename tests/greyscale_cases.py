"""The greyscale rule restated in numpy, and the frames the CPU and GPU tests share.

The rule (the reference's is_greyscale_image): an [H,W,3] uint8 BGR frame is greyscale iff max(b - g) <= 3, max(b - r) <= 3 and
max(g - r) <= 3, where b, g, r are uint8 views - so each difference wraps modulo 256 before the maximum is taken, b - g = -1 is
255, and in effect a frame passes iff every pixel has r <= g <= b <= r + 3.  mode 'abs' takes |b-g|, |b-r|, |g-r| instead.  A
record holds the three wrapped maxima, the three absolute maxima, a status word and a zero."""
import numpy as np

SIZES = [(2, 16), (6, 48), (7, 50), (3, 17), (1, 1), (5, 15)]        # H, W: the 16-pixel lane, its tail, the bytewise path
WORDS = 8


def records(frames, status=None):
    """uint8 [N,H,W,3] -> int32 [N,8], one pixel difference at a time as the statement above reads."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim == 4 and frames.shape[3] == 3
    out = np.zeros((frames.shape[0], WORDS), np.int32)
    for n, f in enumerate(frames):
        b, g, r = f[:, :, 0], f[:, :, 1], f[:, :, 2]
        for q, (x, y) in enumerate(((b, g), (b, r), (g, r))):
            wrapped = x - y                                         # uint8 - uint8: modulo 256
            assert wrapped.dtype == np.uint8
            out[n, q] = int(wrapped.max())
            out[n, 3 + q] = int(np.abs(x.astype(np.int32) - y.astype(np.int32)).max())
    if status is not None:
        out[:, 6] = status
    return out


def is_greyscale(rec, threshold=3, mode="reference"):
    lo = {"reference": 0, "abs": 3}[mode]
    return (np.asarray(rec)[..., lo:lo + 3] <= threshold).all(-1)


def is_greyscale_by_pixels(frame, threshold=3):
    """The 'in effect' form of the reference rule: every pixel has r <= g <= b <= r + threshold."""
    b, g, r = (frame[..., c].astype(np.int32) for c in range(3))
    return bool(((r <= g) & (g <= b) & (b <= r + threshold)).all())


def random_frames(seed, N, H, W, near_grey=True):
    """near_grey: b, g, r within a few code values of each other in both directions, so that maxima on both sides of the threshold
    and wrapped values all occur; else uniform bytes."""
    rng = np.random.default_rng(seed)
    if not near_grey:
        return rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    v = rng.integers(0, 250, (N, H, W, 1))
    d = rng.integers(0, 4, (N, H, W, 3))
    d[..., 2] = 0
    d[..., 0] = np.maximum(d[..., 0], d[..., 1])                     # r <= g <= b <= r + 3: greyscale so far
    f = (v + d).astype(np.uint8)
    for n in range(0, N, 2):                                         # every other frame gets one pixel that breaks the order
        f[n, rng.integers(H), rng.integers(W)] = (10, 11 + n % 3, 10)
    return f


# (name, (db, dg, dr) added to the pixel's base value, greyscale under 'reference', under 'abs')
PIXELS = [
    ("b+3", (3, 0, 0), True, True),            # b-g = b-r = 3
    ("b+4", (4, 0, 0), False, False),          # b-g = b-r = 4
    ("g+1", (0, 1, 0), False, True),           # b-g = -1 wraps to 255; |b-g| = 1
    ("b-r=3", (3, 1, 0), True, True),          # b-g 2, b-r 3, g-r 1
    ("b-r=4", (4, 2, 0), False, False),        # b-g 2, b-r 4, g-r 2: b-r alone is over
    ("g-r=3", (3, 3, 0), True, True),          # b-g 0, b-r 3, g-r 3
    ("g-r=4", (4, 4, 0), False, False),        # g-r 4 (and with it b-r)
    ("r+1", (0, 0, 1), False, True),           # b-r = g-r = -1 wrap to 255
    ("r+4", (0, 0, 4), False, False),          # wrapped 252, absolute 4
]
BASES = [0, 100, 252]


def positions(H, W):
    """Flat pixel indices: the first pixel, the last pixel of the last row, the last pixel of a lane's 16, the first pixel of the
    tail (the pixels behind the last whole 16), the first pixel of the last row and the last column of the first row."""
    n = H * W
    want = [0, n - 1, 15, (n // 16) * 16, (H - 1) * W, W - 1, 16]
    return sorted({p for p in want if 0 <= p < n})


def single_pixel_frames(H, W):
    """-> (frames uint8 [N,H,W,3], cases [(name, v, flat position, grey under 'reference', grey under 'abs')]): every frame grey
    v,v,v but for one pixel.  The pixel's own base is lowered where v + offset would pass 255, so the differences stay as named."""
    frames, cases = [], []
    for v in BASES:
        for name, off, ref, ab in PIXELS:
            for p in positions(H, W):
                f = np.full((H * W, 3), v, np.uint8)
                base = min(v, 255 - max(off))
                f[p] = [base + o for o in off]
                frames.append(f.reshape(H, W, 3))
                cases.append((name, v, p, ref, ab))
    return np.stack(frames), cases
