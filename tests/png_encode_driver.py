"""ctypes binding of the host build of csrc/png_deflate.h (csrc/png_encode_host.cpp, make png_encode_host) and the encoder's
test corpus.  The host build runs the code the GPU runs, one lane at a time, and must give the same bytes: the CPU tests
(tests/test_png_encode_cpu.py) check those bytes against zlib, Pillow and tests/png_corpus.py, the GPU tests
(tests/test_gpu_png_encode.py) check the device against them."""
import ctypes as C
import functools
import os
import subprocess
import zlib

import numpy as np

from tests import png_corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "relax-vqa_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
OK, BAD_ARGS, OUT_TOO_SMALL = 0, 1, 14
SHAPES = [(1, 1), (1, 3), (5, 3), (9, 17), (12, 224), (224, 224), (3, 1920), (2, 5461)]
RUNS = (1, 2, 3, 4, 257, 258, 259, 260, 261, 517)
_lib = None


def load():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-C", CSRC, "librelax_png_encode_host.so"], check=True, capture_output=True)   # a no-op when up to date
        lib = C.CDLL(os.path.join(CSRC, "librelax_png_encode_host.so"))
        lib.relax_png_encode_bound_host.restype = C.c_int64
        lib.relax_png_encode_bound_host.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_int64), C.POINTER(C.c_int)]
        lib.relax_png_encode_host.restype = C.c_int
        lib.relax_png_encode_host.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                              C.c_void_p, C.c_void_p]
        lib.relax_png_deflate_host.restype = C.c_int64
        lib.relax_png_deflate_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
        _lib = lib
    return _lib


def bound(H, W, Cc, filt=-1, lib_fn=None):
    """-> (stream bound, scratch bytes, rows per band), or None for a refused geometry."""
    scratch, rows = C.c_int64(0), C.c_int(0)
    b = (lib_fn or load().relax_png_encode_bound_host)(H, W, Cc, filt, C.byref(scratch), C.byref(rows))
    return None if b < 0 else (int(b), int(scratch.value), int(rows.value))


def channels(img):
    return 1 if img.ndim == 2 else img.shape[2]


def layout(imgs, filters, capacities=None):
    """The buffers of one call: (images uint8, items int64 [N,8], out bytes, scratch bytes).  capacities: per image, None = the
    bound.  A refused geometry gets capacity 0 and takes no scratch."""
    items = np.zeros((len(imgs), 8), np.int64)
    at = out_at = scratch = 0
    for n, (img, f) in enumerate(zip(imgs, filters)):
        H, W, Cc = img.shape[0], img.shape[1], channels(img)
        g = bound(H, W, Cc, f)
        cap = (g[0] if g else 0) if capacities is None or capacities[n] is None else capacities[n]
        items[n] = (at, W * Cc, H, W, Cc, out_at, cap, f)
        at += img.size
        out_at += (cap + 7) // 8 * 8
        scratch += g[1] if g else 128
    flat = np.concatenate([np.ascontiguousarray(i).reshape(-1) for i in imgs]) if imgs else np.zeros(0, np.uint8)
    return flat, items, max(out_at, 8), scratch


def encode_host(imgs, filters=None, capacities=None, scratch_fill=0xFF):
    """-> (streams: bytes per image or None, lengths, statuses) of relax_png_encode_host."""
    filters = [-1] * len(imgs) if filters is None else list(filters)
    flat, items, out_bytes, scratch_bytes = layout(imgs, filters, capacities)
    out = np.full(out_bytes, 0xEE, np.uint8)
    scratch = np.full(scratch_bytes, scratch_fill, np.uint8)
    lengths = np.full(len(imgs), -1, np.int64)
    status = np.full(len(imgs), -1, np.int32)
    rc = load().relax_png_encode_host(flat.ctypes.data, flat.size, items.ctypes.data, len(imgs), out.ctypes.data, out.size,
                                      scratch.ctypes.data, scratch.size, lengths.ctypes.data, status.ctypes.data)
    assert rc == 0, f"relax_png_encode_host refused the call ({rc})"
    streams = [bytes(out[items[n, 5]:items[n, 5] + lengths[n]]) if status[n] == 0 else None for n in range(len(imgs))]
    return streams, lengths, status, out, items


def deflate_raw(raw):
    """The deflate core alone on raw bytes (one band) -> zlib stream."""
    raw = np.frombuffer(bytes(raw), np.uint8)
    out = np.zeros(raw.size + 16, np.uint8)
    n = load().relax_png_deflate_host(raw.ctypes.data, raw.size, out.ctypes.data, out.size)
    assert n > 0
    return bytes(out[:n])


# ---- reference arithmetic ---------------------------------------------------------------------------------------------------
def png_rows(img):
    """BGR / gray pixels -> the PNG's raw rows uint8 [H, W*C] (RGB order) and bytes per pixel."""
    if img.ndim == 2:
        return img, 1
    return np.ascontiguousarray(img[..., ::-1]).reshape(img.shape[0], -1), 3


def adaptive_filters(img):
    """Per row the filter with the smallest sum of |filtered byte read as signed|, ties to the lowest number (libpng's
    heuristic), recomputed with tests/png_corpus.filter_rows."""
    rows, bpp = png_rows(img)
    H, n = rows.shape
    sums = np.zeros((5, H), np.int64)
    for f in range(5):
        filt = np.frombuffer(png_corpus.filter_rows(rows, bpp, [f] * H), np.uint8).reshape(H, n + 1)[:, 1:].astype(np.int64)
        sums[f] = np.where(filt < 128, filt, 256 - filt).sum(axis=1)
    return np.argmin(sums, axis=0)


def expected_raw(img, filt):
    rows, bpp = png_rows(img)
    filters = adaptive_filters(img) if filt < 0 else [filt] * rows.shape[0]
    return png_corpus.filter_rows(rows, bpp, filters)


class Bits:
    def __init__(self, data, at):
        self.d, self.pos = data, at * 8

    def take(self, n):
        v = 0
        for i in range(n):
            v |= ((self.d[self.pos >> 3] >> (self.pos & 7)) & 1) << i
            self.pos += 1
        return v


def _decoder(lengths):
    table, code = {}, 0
    for l in range(1, 16):
        for sym, sl in enumerate(lengths):
            if sl == l:
                table[(l, code)] = sym
                code += 1
        code <<= 1
    return table


def _symbol(b, table):
    code = 0
    for l in range(1, 16):
        code = (code << 1) | b.take(1)
        if (l, code) in table:
            return table[(l, code)]
    raise AssertionError("no such code")


def blocks(z):
    """Walks a zlib stream block by block -> [dict(type, final, size (bytes of a stored block), lit_lengths, dist_lengths)].
    A small inflate of its own (dynamic and stored blocks), so the block structure is checked without the code under test."""
    b = Bits(z, 2)
    out = []
    while True:
        final, btype = b.take(1), b.take(2)
        info = dict(type=btype, final=final)
        if btype == 0:
            b.pos = (b.pos + 7) // 8 * 8
            ln, nln = b.take(16), b.take(16)
            assert ln ^ 0xFFFF == nln
            b.pos += 8 * ln
            info["size"] = ln
        else:
            assert btype == 2, "the encoder writes stored and dynamic blocks only"
            hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
            cl = [0] * 19
            for i in range(hclen):
                cl[(16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)[i]] = b.take(3)
            ct = _decoder(cl)
            lens = []
            while len(lens) < hlit + hdist:
                s = _symbol(b, ct)
                if s < 16:
                    lens.append(s)
                elif s == 16:
                    lens += [lens[-1]] * (3 + b.take(2))
                elif s == 17:
                    lens += [0] * (3 + b.take(3))
                else:
                    lens += [0] * (11 + b.take(7))
            info["lit_lengths"], info["dist_lengths"] = lens[:hlit], lens[hlit:]
            lt, dt = _decoder(lens[:hlit]), _decoder(lens[hlit:])
            while True:
                s = _symbol(b, lt)
                if s == 256:
                    break
                if s > 256:
                    s -= 257
                    if 8 <= s < 28:
                        b.take((s - 4) >> 2)
                    d = _symbol(b, dt)
                    if d >= 4:
                        b.take((d - 2) >> 1)
        out.append(info)
        if final:
            return out


# ---- the corpus -------------------------------------------------------------------------------------------------------------
def content(kind, H, W, Cc, seed=0):
    rng = np.random.default_rng(1234 + seed)           # PCG64
    shape = (H, W) if Cc == 1 else (H, W, 3)
    y, x = np.mgrid[0:H, 0:W]
    if kind == "constant":
        img = np.full(shape, 77)
    elif kind == "hgrad":
        img = x * 3 if Cc == 1 else np.stack([x * 3 + 40 * k for k in range(3)], -1)
    elif kind == "vgrad":
        img = y * 5 if Cc == 1 else np.stack([y * 5 + k for k in range(3)], -1)
    elif kind == "antidiag":                           # x - y: Average (and Paeth) predict it exactly, Sub and Up do not
        img = x - y if Cc == 1 else np.stack([x - y + 9 * k for k in range(3)], -1)
    elif kind == "small":                              # bytes of small absolute value and no structure: None wins
        img = rng.choice(np.array([255, 0, 1]), size=shape)
    elif kind == "noise":
        img = rng.integers(0, 256, shape)
    elif kind == "runs":                               # zero runs of the lengths RUNS between distinct bytes (forced filter 0)
        flat = np.zeros(H * W * Cc, np.int64)
        at, k = 0, seed
        while at < flat.size:
            flat[at] = 1 + k % 255
            at += 1 + RUNS[k % len(RUNS)]
            k += 1
        img = flat.reshape(H, W * Cc) if Cc == 1 else flat.reshape(H, W, 3)
    elif kind == "mixed":
        img = png_corpus.image(H, W, Cc, seed)
        img = img[..., 0] if Cc == 1 else img
    else:
        raise ValueError(kind)
    return np.ascontiguousarray((np.asarray(img) & 255).astype(np.uint8).reshape(shape))


@functools.lru_cache(None)
def golden_frames():
    from PIL import Image
    out = []
    for stem in ("5636101558_3", "TelevisionClip_1080P-68c6_1"):
        with Image.open(os.path.join(GOLDEN, "png_" + stem, stem + ".png")) as im:
            out.append(np.ascontiguousarray(np.asarray(im.convert("RGB"))[..., ::-1]))
    return out


def golden_crop(H, W, Cc, k):
    frame = golden_frames()[1 if W > golden_frames()[0].shape[1] else k % 2]       # the 1080p frame where the other is too narrow
    fh, fw = frame.shape[:2]
    y0, x0 = (37 + 151 * k) % max(fh - H, 1), (11 + 97 * k) % max(fw - W, 1)
    crop = frame[y0:y0 + H, x0:x0 + W]
    assert crop.shape[:2] == (H, W)
    return np.ascontiguousarray(crop if Cc == 3 else crop[..., 1])


def three_band_shape(Cc, W=224):
    """(H, W) with three bands and a shorter last one, from the rows per band relax_png_encode_bound reports."""
    rows = bound(1, W, Cc)[2]
    return 2 * rows + (rows + 1) // 2, W


@functools.lru_cache(None)
def cases():
    """-> tuple of (name, image, filter): every shape, gray and BGR, with every content kind; forced filters 0-4; golden crops."""
    out = []
    k = 0
    for Cc in (1, 3):
        for H, W in SHAPES + [three_band_shape(Cc)]:
            tag = f"{'gray' if Cc == 1 else 'bgr'}_{H}x{W}"
            for kind in ("constant", "hgrad", "vgrad", "antidiag", "small", "noise"):
                out.append((f"{kind}_{tag}", content(kind, H, W, Cc, k), -1))
                k += 1
            out.append((f"runs_{tag}", content("runs", H, W, Cc, k), 0))
            for f in range(5):
                out.append((f"mixed_f{f}_{tag}", content("mixed", H, W, Cc, k), f))
                k += 1
    # crops of the golden frames.  Every one must come out smaller than its pixels (tests/test_png_encode_cpu.py), and a dynamic
    # block spends about 150 bytes per band on its header before the first pixel, whatever the crop holds; so the crops start at
    # 12 x 224 (2688 bytes of pixels and more), the smallest shape of the list with room for a header beside real image noise.
    g = 0
    for Cc in (1, 3):
        for H, W in ((12, 224), (224, 224), (224, 224), (3, 1920), (6, 960), three_band_shape(Cc)):
            out.append((f"golden{g}_{'gray' if Cc == 1 else 'bgr'}_{H}x{W}", golden_crop(H, W, Cc, g), -1))
            g += 1
    # histograms that want more than 15 bits, as images of one band under forced filter 0 (see fibonacci_bytes, skewed_bytes)
    out.append(("fibonacci_gray_2x8855", fibonacci_bytes().reshape(2, 8855), 0))
    out.append(("skewed_gray_7x2526", skewed_bytes(as_image=True), 0))
    return tuple(out)


@functools.lru_cache(None)
def host_results():
    """The host build's streams for cases(), one call: computed once and shared."""
    cs = cases()
    streams, lengths, status, _, _ = encode_host([c[1] for c in cs], [c[2] for c in cs])
    return streams, lengths, status


def fibonacci_bytes():
    """Value k appears F(k) times, k = 1..20 (F = 1, 1, 2, 3, ...: 17710 bytes), shuffled by a fixed seed."""
    fib = [1, 1]
    while len(fib) < 20:
        fib.append(fib[-1] + fib[-2])
    raw = np.concatenate([np.full(f, k + 1, np.uint8) for k, f in enumerate(fib)])
    np.random.default_rng(20).shuffle(raw)
    return raw


def skewed_counts():
    """w(k) = w(k-1) + w(k-2) + 1 from 2, 4: 17 counts without Fibonacci's ties, 17689 = 133 * 133 bytes in all.  An unlimited
    Huffman code of them (plus end-of-block) is 17 bits deep."""
    w = [2, 4]
    while len(w) < 17:
        w.append(w[-1] + w[-2] + 1)
    return w


def skewed_bytes(as_image=False):
    """Value k + 1 appears skewed_counts()[k] times and no two neighbours are equal: every byte is a literal, so the histogram
    reaches the code builder as it is and the 15-bit limit is hit.  as_image: a gray [7, 2526] image of the same histogram under
    forced filter 0 - the value with the count 7 is left out of the pixels and the seven filter bytes (0) take its place."""
    counts = skewed_counts()
    by_count = np.concatenate([np.full(c, k + 1, np.uint8) for k, c in enumerate(counts) if not (as_image and c == 7)])[::-1]
    out = np.empty_like(by_count)
    half = (by_count.size + 1) // 2
    out[0::2], out[1::2] = by_count[:half], by_count[half:]
    assert (out[1:] != out[:-1]).all()
    return out.reshape(7, 2526) if as_image else out


def size_parity():
    """Our stream against zlib's Z_RLE at level 6 over the encoder's own filtered bytes, for the golden crops and the gradients
    -> {case: ratio}."""
    cs = cases()
    streams = host_results()[0]
    out = {}
    for (name, img, f), z in zip(cs, streams):
        if name.split("_")[0] in ("hgrad", "vgrad", "antidiag") or name.startswith("golden"):
            raw = zlib.decompress(z)
            co = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_RLE)
            ref = co.compress(raw) + co.flush()
            out[name] = len(z) / len(ref)
    return out
