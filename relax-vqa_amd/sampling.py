"""Frame-sampling semantics and on-disk feature formats of the reference, without ffmpeg: the caller
decodes the video (or already holds the frames) and these helpers reproduce which frames the reference's ffmpeg
`select` filters pick, how they are paired, and how per-clip features are named and packed.

  frame_interval          src/main_fragment_layerstack.py:274-277   (2 samples per second)
  sampled_frame_indices   src/video_frames_extract.py:12-20 (not(mod(n,k))), :61-66 (not(mod(n-1,k))), pairing by sorted
                          index with zip truncation src/main_fragment_layerstack.py:283-293
  frame_pair_paths / load_clip_from_frames   src/main_fragment_layerstack.py:283-296: the sampled frames the reference's ffmpeg step left on disk
                          (`{video}_{n}.png`, `{video}_{n}_next.png`), paired by sorted index, read as cv2.imread reads them (uint8 BGR)
  yuv_format / yuv_samples / yuv_frame_bgr_ex   the same for 10 / 12-bit, packed 4:2:2, 4:1:1, 4:1:0 and NV21 input (extended=True)
  yuv_layout / yuv_frame_count / yuv_frame_bgr / load_clip_from_yuv / GpuYuvLoader   src/video_frames_extract.py:29-49,76-100: the frames
                          ffmpeg cuts out of headerless raw video (`-s WxH -pix_fmt yuv420p -framerate r -i file.yuv`, the live_qualcomm
                          input path), converted from the file's own bytes by the integer formula of include/relax_hip.h
  feature_file_name       src/main_fragment_layerstack.py:67-68,349-354  video_{i+1}_{network}_feature_map_original.npy
  features_matrix / save_mat  src/data_processing/extract_npy2mat.py:117-130, 79-84 (np.mean over frames; .mat key = dataset)
"""
import math
import os
import threading

import numpy as np


def frame_interval(framerate):
    return math.ceil(framerate / 2) if framerate < 2 else int(framerate / 2)


def sampled_frame_indices(n_frames, interval):
    """-> (sampled, following, pairs): frames n with n % k == 0, frames n with (n-1) % k == 0, and the (frame, next)
    index pairs the drivers zip together (truncated to the shorter list)."""
    k = max(int(interval), 1)
    sampled = [n for n in range(n_frames) if n % k == 0]
    following = [n for n in range(n_frames) if (n - 1) % k == 0]
    return sampled, following, list(zip(sampled, following))


def pair_frames(video_frames, framerate):
    """video_frames uint8 [N,H,W,3] (decoded, BGR) -> uint8 [T,2,H,W,3] as relax_fragment_pairs expects."""
    _, _, pairs = sampled_frame_indices(len(video_frames), frame_interval(framerate))
    if not pairs:
        return np.empty((0, 2) + tuple(video_frames.shape[1:]), dtype=video_frames.dtype)
    return np.stack([np.stack([video_frames[a], video_frames[b]]) for a, b in pairs])


def frame_pair_paths(sampled_frame_path, video_name):
    """-> [(frame path, next-frame path), ...] as the reference pairs them (src/main_fragment_layerstack.py:283-293):
    `{video_name}_{n}.png` sorted by n, `{video_name}_{n}_next.png` sorted by n, zipped (the longer list is truncated)."""
    import glob
    base = glob.escape(os.path.join(sampled_frame_path, video_name))
    originals = sorted((p for p in glob.glob(base + "_*.png") if "_next" not in os.path.basename(p)),
                       key=lambda x: int(x.split("_")[-1].split(".")[0]))
    following = sorted(glob.glob(base + "_*_next.png"), key=lambda x: int(x.split("_")[-2]))
    return list(zip(originals, following))


def read_frame_bgr(path):
    """A frame file as `cv2.imread(path)` returns it (src/main_fragment_layerstack.py:295-296): uint8 [H,W,3], BGR, alpha dropped,
    gray replicated.  Decoded with Pillow (the GIL is released while it decodes: loader threads read frames in parallel)."""
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[..., ::-1])


def load_clip_from_frames(sampled_frame_path, video_name, alloc=None):
    """The sampled frames of one video on disk -> uint8 [T,2,H,W,3] BGR, the input of relax_fragment_pairs / of
    dataset.extract_dataset_clips (as its `clips(i)` callable: the decode then runs in the loader threads, ahead of the engine).
    alloc (the dataset driver's protocol): shape -> the uint8 array to fill - pinned staging memory: every frame is decoded and
    written straight into its slot of the clip, no pageable copy of the clip is made.
    Raises if the directory holds no pair or the frames differ in size."""
    pairs = frame_pair_paths(sampled_frame_path, video_name)
    if not pairs:
        raise FileNotFoundError(f"no `{video_name}_<n>.png` / `{video_name}_<n>_next.png` pair under {sampled_frame_path}")
    first = read_frame_bgr(pairs[0][0])
    shape = first.shape
    out = (alloc or np.empty)((len(pairs), 2) + shape) if alloc is not None else np.empty((len(pairs), 2) + shape, dtype=np.uint8)
    for t, (pa, pb) in enumerate(pairs):
        for j, path in enumerate((pa, pb)):
            f = first if (t == 0 and j == 0) else read_frame_bgr(path)
            if f.shape != shape:
                raise ValueError(f"{pa} / {pb}: frame sizes differ inside one video ({f.shape} vs {shape})")
            out[t, j] = f
    return out


class GpuFrameLoader:
    """load_clip_from_frames on the GPU: clip i -> the uint8 BGR device tensor [T,2,H,W,3] that
    load_clip_from_frames(sampled_frame_path, names[i]) returns on the host, byte for byte (same pairing, same errors).  The
    files are read and their containers parsed on the calling thread; the image data is decoded by relax_png_decode on that
    thread's own stream (pngdecode.decoder_for), so loader threads decode at the same time.  Pass it as the `clips` of
    dataset.extract_dataset_clips, which uses device tensors as they are.  The clip is complete when __call__ returns and is
    recorded on `consumer_stream` (default: the current stream of `device` when the loader is made - the stream the dataset
    pass computes on).  A file the decoder refuses raises (in a dataset pass: that clip's NaN row and error entry).
    fallbacks: how many files so far were decoded on the host (16-bit, palette, gray + alpha, interlaced)."""

    def __init__(self, sampled_frame_path, names, device=None, consumer_stream=None):
        import torch
        self.path = sampled_frame_path
        self.names = list(names)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.consumer = consumer_stream if consumer_stream is not None else torch.cuda.current_stream(self.device)
        self.fallbacks = 0
        self._lock = threading.Lock()

    def __len__(self):
        return len(self.names)

    def __call__(self, i):
        import torch

        from . import png, pngdecode
        name = self.names[i]
        pairs = frame_pair_paths(self.path, name)
        if not pairs:
            raise FileNotFoundError(f"no `{name}_<n>.png` / `{name}_<n>_next.png` pair under {self.path}")
        parsed = []
        for pa, pb in pairs:
            for path in (pa, pb):
                src, data = png.read_source(path)
                parsed.append((src, png.parse(data, src)))
        shape = parsed[0][1].shape
        for t, (pa, pb) in enumerate(pairs):
            for j in (0, 1):
                s = parsed[2 * t + j][1].shape
                if s != shape:
                    raise ValueError(f"{pa} / {pb}: frame sizes differ inside one video ({s} vs {shape})")
        dec = pngdecode.decoder_for(self.device)
        with torch.cuda.stream(dec.stream):
            clip = torch.empty((len(pairs), 2) + shape, dtype=torch.uint8, device=self.device)
        stats = {}
        dec.decode(None, out=clip.view((-1,) + shape), parsed=parsed, stats=stats)
        clip.record_stream(self.consumer)
        with self._lock:
            self.fallbacks += stats.get("fallback", 0)
        return clip


# ---- raw YUV video (src/video_frames_extract.py:29-49,76-100) ---------------------------------------------------------------
YUV_420P, YUV_422P, YUV_444P, YUV_NV12 = 0, 1, 2, 3      # RELAX_YUV_* of include/relax_hip.h
YUV_MAX_DIM = 16384
YUV_MATRICES = {"bt601": 0, "bt709": 1}
_yuv_coef_cache = {}


def yuv_coefficients(matrix="bt601", full_range=False):
    """(cy, oy, crv, cbu, cgu, cgv) of include/relax_hip.h's formula, read from the library (relax_yuv_coefficients: the one table
    in csrc/yuv_core.h that the kernel uses), so host and device cannot drift apart."""
    key = (matrix, bool(full_range))
    if key not in _yuv_coef_cache:
        import ctypes as C

        from . import _lib
        if matrix not in YUV_MATRICES:
            raise ValueError(f"matrix {matrix!r} is not one of {', '.join(YUV_MATRICES)}")
        out = (C.c_int32 * 6)()
        if _lib.load().relax_yuv_coefficients(YUV_MATRICES[matrix], int(key[1]), out) != 0:
            raise RuntimeError(f"relax_yuv_coefficients refused {key}")
        _yuv_coef_cache[key] = tuple(out)
    return _yuv_coef_cache[key]


_YUV_PIXFMTS = {
    "yuv420p": (YUV_420P, False), "yuvj420p": (YUV_420P, True),
    "yuv422p": (YUV_422P, False), "yuvj422p": (YUV_422P, True),
    "yuv444p": (YUV_444P, False), "yuvj444p": (YUV_444P, True),
    "nv12": (YUV_NV12, False),
}


def yuv_layout(pixfmt):
    """The reference's metadata `pixfmt` string -> (layout, full_range).  8-bit planar 4:2:0 / 4:2:2 / 4:4:4 (yuvj*: full range) and
    nv12; everything else (10-bit and deeper, packed 4:2:2, palette, RGB, ...) raises a ValueError naming it."""
    try:
        return _YUV_PIXFMTS[str(pixfmt).strip()]
    except KeyError:
        raise ValueError(f"pixfmt {pixfmt!r} is not supported: raw input is read as one of {', '.join(_YUV_PIXFMTS)}") from None


def yuv_plan(layout, H, W):
    """The frame layout (csrc/yuv_core.h's Plan, restated): dict of cw, ch (chroma plane size: halves rounded up), u_off, v_off,
    c_stride (bytes between chroma rows), c_step (bytes between chroma samples), frame_bytes."""
    H, W = int(H), int(W)
    if layout not in (YUV_420P, YUV_422P, YUV_444P, YUV_NV12):
        raise ValueError(f"layout {layout!r} is not one of 0..3")
    if not (1 <= H <= YUV_MAX_DIM and 1 <= W <= YUV_MAX_DIM):
        raise ValueError(f"frame size {W}x{H} outside 1..{YUV_MAX_DIM}")
    cw = W if layout == YUV_444P else (W + 1) // 2
    ch = (H + 1) // 2 if layout in (YUV_420P, YUV_NV12) else H
    nv12 = layout == YUV_NV12
    return {"cw": cw, "ch": ch, "u_off": H * W, "v_off": H * W + (1 if nv12 else ch * cw), "c_stride": cw * (2 if nv12 else 1),
            "c_step": 2 if nv12 else 1, "frame_bytes": H * W + 2 * ch * cw}


def yuv_frame_bytes(layout, H, W):
    return yuv_plan(layout, H, W)["frame_bytes"]


def yuv_frame_count(path, W, H, pixfmt, extended=False):
    """Frames in a headerless raw file: size // frame bytes; a size that is no whole number of frames raises.  extended: pixfmt is one
    of yuv_format's names."""
    fb = _yuv_source(pixfmt, extended)[2](H, W)
    size = os.path.getsize(path)
    if size % fb:
        raise ValueError(f"{path}: {size} bytes is not a whole number of {W}x{H} {pixfmt} frames of {fb} bytes "
                         f"({size // fb} frames and {size % fb} bytes over)")
    return size // fb


def yuv_planes(frame, layout, H, W):
    """One frame's bytes (uint8 [frame_bytes]) -> (Y [H,W], U [ch,cw], V [ch,cw]) views."""
    p = yuv_plan(layout, H, W)
    frame = np.asarray(frame, np.uint8).reshape(-1)
    if frame.size != p["frame_bytes"]:
        raise ValueError(f"a {W}x{H} frame of layout {layout} has {p['frame_bytes']} bytes, got {frame.size}")
    y = frame[:H * W].reshape(H, W)
    if layout == YUV_NV12:
        uv = frame[H * W:].reshape(p["ch"], p["cw"], 2)
        return y, uv[..., 0], uv[..., 1]
    n = p["ch"] * p["cw"]
    return y, frame[H * W:H * W + n].reshape(p["ch"], p["cw"]), frame[H * W + n:].reshape(p["ch"], p["cw"])


def yuv_frame_bgr(y, u, v, matrix="bt601", full_range=False, out=None):
    """The numpy statement of relax_yuv_to_bgr's arithmetic (include/relax_hip.h): Y uint8 [H,W], U and V uint8 [ch,cw] with
    ch in (H, ceil(H/2)) and cw in (W, ceil(W/2)) - chroma is replicated, pixel (r, c) takes sample (r >> 1, c >> 1) where the
    plane is halved - -> uint8 [H,W,3] BGR.  int32 throughout; >> is numpy's arithmetic shift."""
    cy, oy, crv, cbu, cgu, cgv = yuv_coefficients(matrix, full_range)
    y = np.asarray(y)
    H, W = y.shape

    def full(c):
        c = np.asarray(c)
        if c.shape[0] != H:
            if c.shape[0] != (H + 1) // 2:
                raise ValueError(f"chroma plane of {c.shape[0]} rows under {H} luma rows")
            c = np.repeat(c, 2, axis=0)[:H]
        if c.shape[1] != W:
            if c.shape[1] != (W + 1) // 2:
                raise ValueError(f"chroma plane of {c.shape[1]} columns under {W} luma columns")
            c = np.repeat(c, 2, axis=1)[:, :W]
        return c.astype(np.int32) - 128

    yy = cy * (y.astype(np.int32) - oy) + (1 << 15)
    uu, vv = full(u), full(v)
    out = np.empty((H, W, 3), np.uint8) if out is None else out
    out[..., 2] = np.clip((yy + crv * vv) >> 16, 0, 255)
    out[..., 1] = np.clip((yy - cgu * uu - cgv * vv) >> 16, 0, 255)
    out[..., 0] = np.clip((yy + cbu * uu) >> 16, 0, 255)
    return out


# ---- the RELAX_YUVF_* formats: 10 / 12-bit, packed 4:2:2, 4:1:1, 4:1:0, NV21 (include/relax_hip.h; opt-in: extended=True) ----------
(YUVF_420P, YUVF_422P, YUVF_444P, YUVF_NV12, YUVF_NV21, YUVF_YUYV422, YUVF_UYVY422, YUVF_411P, YUVF_410P, YUVF_420P10LE, YUVF_422P10LE,
 YUVF_444P10LE, YUVF_420P12LE, YUVF_422P12LE, YUVF_444P12LE, YUVF_P010LE) = range(16)
YUV_PLANAR, YUV_SEMIPLANAR, YUV_PACKED = 0, 1, 2
_YUV_FORMATS = dict(_YUV_PIXFMTS)
_YUV_FORMATS.update({
    "nv21": (YUVF_NV21, False), "yuyv422": (YUVF_YUYV422, False), "uyvy422": (YUVF_UYVY422, False),
    "yuv411p": (YUVF_411P, False), "yuv410p": (YUVF_410P, False),
    "yuv420p10le": (YUVF_420P10LE, False), "yuv422p10le": (YUVF_422P10LE, False), "yuv444p10le": (YUVF_444P10LE, False),
    "yuv420p12le": (YUVF_420P12LE, False), "yuv422p12le": (YUVF_422P12LE, False), "yuv444p12le": (YUVF_444P12LE, False),
    "p010le": (YUVF_P010LE, False),
})
_yuv_info_cache = {}


def yuv_format(pixfmt):
    """The reference's metadata `pixfmt` string -> (format, full_range) for the `_ex` entries: yuv_layout's seven names (formats
    0..3) and nv21, yuyv422, uyvy422, yuv411p, yuv410p, yuv4{20,22,44}p1{0,2}le, p010le.  Everything else (pal8, RGB, alpha,
    big-endian, 14 / 16-bit, gray, ...) raises a ValueError naming it."""
    try:
        return _YUV_FORMATS[str(pixfmt).strip()]
    except KeyError:
        raise ValueError(f"pixfmt {pixfmt!r} is not supported: raw input is read as one of {', '.join(_YUV_FORMATS)}") from None


def yuv_format_info(format):
    """The library's format table (relax_yuv_format_info: csrc/yuv_core.h's, the one the kernels use): dict of sample_bytes, depth,
    shift (sample = (word >> shift) & (2^depth - 1)), hshift, vshift, packing (YUV_PLANAR / YUV_SEMIPLANAR / YUV_PACKED), swap
    (semi-planar: V first; packed: chroma first)."""
    if isinstance(format, bool) or not isinstance(format, (int, np.integer)):
        raise ValueError(f"format {format!r} is not one of RELAX_YUVF_* (0..15)")
    format = int(format)
    if format not in _yuv_info_cache:
        import ctypes as C

        from . import _lib
        out = (C.c_int32 * 8)()
        if _lib.load().relax_yuv_format_info(format, out) != 0:
            raise ValueError(f"format {format!r} is not one of RELAX_YUVF_* (0..15)")
        _yuv_info_cache[format] = dict(zip(("sample_bytes", "depth", "shift", "hshift", "vshift", "packing", "swap"), out))
    return _yuv_info_cache[format]


def yuv_plan_ex(format, H, W):
    """The frame layout of a format, from yuv_format_info's table (csrc/yuv_core.h's plan_ex, restated): dict of cw, ch (chroma plane
    size: W >> hshift and H >> vshift, rounded up), frame_bytes, and the byte offsets / steps / strides of the luma and chroma samples
    (y_off, y_step, y_stride, u_off, v_off, c_step, c_stride)."""
    t = yuv_format_info(format)
    H, W = int(H), int(W)
    if not (1 <= H <= YUV_MAX_DIM and 1 <= W <= YUV_MAX_DIM):
        raise ValueError(f"frame size {W}x{H} outside 1..{YUV_MAX_DIM}")
    sb = t["sample_bytes"]
    cw, ch = -(-W // (1 << t["hshift"])), -(-H // (1 << t["vshift"]))
    if t["packing"] == YUV_PACKED:
        u = 0 if t["swap"] else 1
        return {"cw": cw, "ch": ch, "y_off": 1 if t["swap"] else 0, "y_step": 2, "y_stride": 4 * cw, "u_off": u, "v_off": u + 2, "c_step": 4,
                "c_stride": 4 * cw, "frame_bytes": 4 * cw * H}
    yb, cb = H * W * sb, ch * cw * sb
    p = {"cw": cw, "ch": ch, "y_off": 0, "y_step": sb, "y_stride": W * sb, "frame_bytes": yb + 2 * cb}
    if t["packing"] == YUV_SEMIPLANAR:
        p.update(u_off=yb + (sb if t["swap"] else 0), v_off=yb + (0 if t["swap"] else sb), c_step=2 * sb, c_stride=2 * cw * sb)
    else:
        p.update(u_off=yb, v_off=yb + cb, c_step=sb, c_stride=cw * sb)
    return p


def yuv_frame_bytes_ex(format, H, W):
    return yuv_plan_ex(format, H, W)["frame_bytes"]


def yuv_samples(frame, format, H, W):
    """One frame's bytes (uint8 [frame_bytes]) -> (Y [H,W], U [ch,cw], V [ch,cw], depth): integer arrays at the format's native depth
    (uint8 views for 8-bit planes, uint16 otherwise; shift and mask applied: garbage above a 10-bit value or below a P010 value is gone)."""
    t, p = yuv_format_info(format), yuv_plan_ex(format, H, W)
    H, W = int(H), int(W)
    frame = np.asarray(frame, np.uint8).reshape(-1)
    if frame.size != p["frame_bytes"]:
        raise ValueError(f"a {W}x{H} frame of format {format} has {p['frame_bytes']} bytes, got {frame.size}")
    sb, cw, ch = t["sample_bytes"], p["cw"], p["ch"]

    def plane(off, rows, cols, stride, step):
        at = off + np.arange(rows, dtype=np.int64)[:, None] * stride + np.arange(cols, dtype=np.int64)[None, :] * step
        if sb == 1:
            return frame[at]
        word = frame[at].astype(np.uint16) | (frame[at + 1].astype(np.uint16) << 8)
        return (word >> t["shift"]) & ((1 << t["depth"]) - 1)
    return (plane(p["y_off"], H, W, p["y_stride"], p["y_step"]), plane(p["u_off"], ch, cw, p["c_stride"], p["c_step"]),
            plane(p["v_off"], ch, cw, p["c_stride"], p["c_step"]), t["depth"])


def yuv_frame_bgr_ex(y, u, v, depth=8, matrix="bt601", full_range=False, out=None):
    """The numpy statement of relax_yuv_to_bgr_ex's arithmetic (include/relax_hip.h), s = depth - 8: Y [H,W], U and V [ch,cw] integer
    arrays at `depth` bits with ch in (H, ceil(H/2), ceil(H/4)) and cw in (W, ceil(W/2), ceil(W/4)) - chroma is replicated - -> uint8
    [H,W,3] BGR.  int32 throughout (depth <= 12 keeps every sum inside it).  At depth 8 this is yuv_frame_bgr bit for bit."""
    if depth not in (8, 10, 12):
        raise ValueError(f"depth {depth!r} is not 8, 10 or 12")
    s = depth - 8
    cy, oy, crv, cbu, cgu, cgv = yuv_coefficients(matrix, full_range)
    y = np.asarray(y)
    H, W = y.shape

    def full(c):
        c = np.asarray(c)
        for axis, n in ((0, H), (1, W)):
            if c.shape[axis] != n:
                k = next((k for k in (2, 4) if c.shape[axis] == -(-n // k)), None)
                if k is None:
                    raise ValueError(f"chroma plane of {c.shape[axis]} {'rows' if axis == 0 else 'columns'} under {n} of luma")
                c = np.repeat(c, k, axis=axis)[:H] if axis == 0 else np.repeat(c, k, axis=axis)[:, :W]
        return c.astype(np.int32) - (128 << s)

    yy = cy * (y.astype(np.int32) - (oy << s)) + (1 << (15 + s))
    uu, vv = full(u), full(v)
    out = np.empty((H, W, 3), np.uint8) if out is None else out
    top = (1 << (24 + s)) - 1
    out[..., 2] = np.clip(yy + crv * vv, 0, top) >> (16 + s)
    out[..., 1] = np.clip(yy - cgu * uu - cgv * vv, 0, top) >> (16 + s)
    out[..., 0] = np.clip(yy + cbu * uu, 0, top) >> (16 + s)
    return out


def _yuv_source(pixfmt, extended):
    """-> (layout or format, full_range, frame_bytes(H, W), frame_bgr(bytes, H, W, matrix, out)) of a pixfmt: the 8-bit surface
    (yuv_layout, relax_yuv_to_bgr), or with extended=True the RELAX_YUVF_* one (yuv_format, the `_ex` entries)."""
    if not extended:
        layout, full_range = yuv_layout(pixfmt)
        return (layout, full_range, lambda H, W: yuv_frame_bytes(layout, H, W),
                lambda buf, H, W, matrix, out: yuv_frame_bgr(*yuv_planes(buf, layout, H, W), matrix=matrix, full_range=full_range, out=out))
    fmt, full_range = yuv_format(pixfmt)

    def frame_bgr(buf, H, W, matrix, out):
        y, u, v, depth = yuv_samples(buf, fmt, H, W)
        return yuv_frame_bgr_ex(y, u, v, depth, matrix=matrix, full_range=full_range, out=out)
    return fmt, full_range, lambda H, W: yuv_frame_bytes_ex(fmt, H, W), frame_bgr


def _yuv_pairs(path, W, H, pixfmt, framerate, extended=False):
    n = yuv_frame_count(path, W, H, pixfmt, extended)
    _, _, pairs = sampled_frame_indices(n, frame_interval(framerate))
    if not pairs:
        raise FileNotFoundError(f"{path}: {n} frames at framerate {framerate} hold no (frame, next frame) pair")
    return pairs


def load_clip_from_yuv(path, W, H, pixfmt, framerate, alloc=None, matrix="bt601", extended=False):
    """A raw YUV video -> uint8 [T,2,H,W,3] BGR: pair_frames() of the converted video, reading only the sampled frames and their
    successors (the PNGs the reference's two ffmpeg passes leave behind, src/video_frames_extract.py:76-100, without the PNGs).
    The host twin of GpuYuvLoader; alloc as in load_clip_from_frames.  Raises FileNotFoundError if the file holds no pair.
    extended=True: pixfmt is one of yuv_format's names and the frames go through yuv_samples / yuv_frame_bgr_ex."""
    _, _, frame_bytes, frame_bgr = _yuv_source(pixfmt, extended)
    pairs = _yuv_pairs(path, W, H, pixfmt, framerate, extended)
    fb = frame_bytes(H, W)
    shape = (len(pairs), 2, int(H), int(W), 3)
    out = alloc(shape) if alloc is not None else np.empty(shape, dtype=np.uint8)
    buf = np.empty(2 * fb, np.uint8)
    with open(path, "rb", buffering=0) as f:
        for t, (a, b) in enumerate(pairs):
            span = b - a + 1                                   # 2: the successor, one read; 1: interval 1 pairs a frame with itself
            f.seek(a * fb)
            if span not in (1, 2) or f.readinto(memoryview(buf[:span * fb])) != span * fb:
                raise OSError(f"{path}: short read at frame {a}")
            for j, n in enumerate((a, b)):
                frame_bgr(buf[(n - a) * fb:(n - a + 1) * fb], H, W, matrix, out[t, j])
    return out


def load_frames_from_yuv(path, W, H, pixfmt, indices, matrix="bt601", extended=False):
    """Frames `indices` of a raw YUV video -> uint8 [len(indices),H,W,3] BGR (host).  extended: as load_clip_from_yuv."""
    _, _, frame_bytes, frame_bgr = _yuv_source(pixfmt, extended)
    n = yuv_frame_count(path, W, H, pixfmt, extended)
    fb = frame_bytes(H, W)
    out = np.empty((len(indices), int(H), int(W), 3), np.uint8)
    buf = np.empty(fb, np.uint8)
    with open(path, "rb", buffering=0) as f:
        for k, i in enumerate(indices):
            if not 0 <= i < n:
                raise IndexError(f"{path}: frame {i} of {n}")
            f.seek(i * fb)
            if f.readinto(memoryview(buf)) != fb:
                raise OSError(f"{path}: short read at frame {i}")
            frame_bgr(buf, H, W, matrix, out[k])
    return out


def read_yuv_frames(path, frames, frame_bytes, slot_bytes, host):
    """Frames `frames` (ascending indices) of a raw file -> host[k * slot_bytes : k * slot_bytes + frame_bytes] for the k-th of
    them (host: a writable uint8 array, the pinned staging buffer).  Each run of adjacent frames is one os.preadv with one
    buffer per frame, so the slots may be padded to an alignment the file's frames do not have.  -> number of reads."""
    reads = 0
    fd = os.open(path, os.O_RDONLY)
    try:
        k = 0
        while k < len(frames):
            e = k + 1
            while e < len(frames) and frames[e] == frames[e - 1] + 1 and e - k < 512:      # (IOV_MAX is 1024)
                e += 1
            views = [memoryview(host[j * slot_bytes:j * slot_bytes + frame_bytes]) for j in range(k, e)]
            want, at = (e - k) * frame_bytes, frames[k] * frame_bytes
            got = os.preadv(fd, views, at)
            reads += 1
            while 0 < got < want:                                   # a short read (signals, network file systems): go on behind it
                rest = [v[max(0, got - j * frame_bytes):] for j, v in enumerate(views) if got < (j + 1) * frame_bytes]
                more = os.preadv(fd, rest, at + got)
                if more <= 0:
                    break
                got += more
            if got != want:
                raise OSError(f"{path}: read {got} of {want} bytes at frame {frames[k]}")
            k = e
    finally:
        os.close(fd)
    return reads


class _YuvThreadState:
    """One loader thread's stream and pinned staging buffer."""

    def __init__(self, device):
        import torch
        self.stream = torch.cuda.Stream(device)
        self.pinned = None

    def staging(self, n):
        import torch
        if self.pinned is None or self.pinned.numel() < n:
            self.pinned = torch.empty(max(n, 1 << 20) * 5 // 4, dtype=torch.uint8, pin_memory=True)
        return self.pinned


class GpuYuvLoader:
    """load_clip_from_yuv on the GPU: clip i -> the uint8 BGR device tensor [T,2,H,W,3] that load_clip_from_yuv(paths[i],
    widths[i], heights[i], pixfmts[i], framerates[i]) returns on the host, byte for byte.  Only the sampled frames and their
    successors are read: each run of adjacent frames is one os.preadv into the calling thread's pinned buffer (every frame at a
    16-byte-aligned slot, so the kernel's 16-byte path applies whenever W is a multiple of 16), followed by one host-to-device
    copy and one relax_yuv_to_bgr launch on that thread's own stream; loader threads work at the same time.  Pass it as the
    `clips` of dataset.extract_dataset_clips.  The clip is complete when __call__ returns and is recorded on `consumer_stream`
    (default: the current stream of `device` when the loader is made).  A file with no pair raises FileNotFoundError.
    extended=True: the pixfmts are yuv_format's names and the launch is relax_yuv_to_bgr_ex; the host twin is
    load_clip_from_yuv(..., extended=True)."""

    def __init__(self, paths, widths, heights, pixfmts, framerates, device=None, consumer_stream=None, matrix="bt601", extended=False):
        import torch

        from . import _lib
        self.paths = list(paths)
        n = len(self.paths)

        def per_clip(v, what):
            v = [v] * n if np.isscalar(v) or isinstance(v, str) else list(v)
            if len(v) != n:
                raise ValueError(f"{len(v)} {what} for {n} paths")
            return v
        self.widths, self.heights = per_clip(widths, "widths"), per_clip(heights, "heights")
        self.pixfmts, self.framerates = per_clip(pixfmts, "pixfmts"), per_clip(framerates, "framerates")
        if matrix not in YUV_MATRICES:
            raise ValueError(f"matrix {matrix!r} is not one of {', '.join(YUV_MATRICES)}")
        self.matrix = matrix
        self.extended = bool(extended)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.consumer = consumer_stream if consumer_stream is not None else torch.cuda.current_stream(self.device)
        self.lib = _lib.load()
        self._tls = threading.local()

    def __len__(self):
        return len(self.paths)

    def _state(self):
        st = getattr(self._tls, "state", None)
        if st is None:
            st = self._tls.state = _YuvThreadState(self.device)
        return st

    def __call__(self, i):
        import ctypes as C

        import torch
        path, W, H = self.paths[i], int(self.widths[i]), int(self.heights[i])
        layout, full_range, frame_bytes, _ = _yuv_source(self.pixfmts[i], self.extended)
        pairs = _yuv_pairs(path, W, H, self.pixfmts[i], self.framerates[i], self.extended)
        fb = frame_bytes(H, W)
        convert, name = (self.lib.relax_yuv_to_bgr_ex, "relax_yuv_to_bgr_ex") if self.extended else (self.lib.relax_yuv_to_bgr, "relax_yuv_to_bgr")
        slot_bytes = (fb + 15) // 16 * 16
        frames = sorted({n for ab in pairs for n in ab})
        slot = {n: k for k, n in enumerate(frames)}
        items_at = len(frames) * slot_bytes
        total = items_at + 16 * 2 * len(pairs)
        st = self._state()
        pinned = st.staging(total)
        host = pinned.numpy()
        read_yuv_frames(path, frames, fb, slot_bytes, host)
        items = np.empty((len(pairs) * 2, 2), np.int64)
        slot_out = H * W * 3
        for t, (a, b) in enumerate(pairs):
            items[2 * t] = (slot[a] * slot_bytes, (2 * t) * slot_out)
            items[2 * t + 1] = (slot[b] * slot_bytes, (2 * t + 1) * slot_out)
        host[items_at:total] = items.view(np.uint8).reshape(-1)
        with torch.cuda.stream(st.stream):
            clip = torch.empty((len(pairs), 2, H, W, 3), dtype=torch.uint8, device=self.device)
            dev = pinned[:total].to(self.device, non_blocking=True)
            status = torch.empty(len(pairs) * 2, dtype=torch.int32, device=self.device)
            rc = convert(C.c_void_p(dev.data_ptr()), items_at, C.c_void_p(dev.data_ptr() + items_at), len(pairs) * 2,
                         layout, H, W, YUV_MATRICES[self.matrix], int(full_range), C.c_void_p(clip.data_ptr()),
                         clip.numel(), C.c_void_p(status.data_ptr()), C.c_void_p(st.stream.cuda_stream))
            if rc != 0:
                raise RuntimeError(f"{name} failed ({rc}): {self.lib.relax_last_error(None).decode()}")
            bad = status.cpu()                                      # waits for the conversion: the pinned buffer is free again
        if bool(bad.any()):
            raise RuntimeError(f"{path}: {name} refused items {bad.nonzero().view(-1).tolist()} (out of range)")
        clip.record_stream(self.consumer)
        return clip


def feature_file_name(video_index, network_name, resolution=None):
    """video_index is 0-based like the reference's loop variable i."""
    name = f"{network_name}_feature_map_original" + (f"_{resolution}" if resolution else "")
    return f"video_{video_index + 1}_{name}.npy"


def save_clip_features(directory, video_index, network_name, per_frame_features, skip_existing=False):
    """np.save of the [T,F] array under the reference's file name; skip_existing gives the resume behaviour the
    reference lacks (SURVEY §5 checkpoint/resume)."""
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, feature_file_name(video_index, network_name))
    if skip_existing and os.path.exists(path):
        return path
    # write under a temporary name, then rename: a run killed mid-write (or a second rank / run reading the directory) never sees
    # a truncated array under the final name (os.replace is atomic within a directory)
    tmp = f"{path}.{os.getpid()}.{threading.get_ident()}.tmp"
    try:
        with open(tmp, "wb") as f:
            np.save(f, np.asarray(per_frame_features))
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return path


def features_matrix(npy_paths):
    """[n_videos, F]: per-video mean over frames (extract_npy2mat.py:117-126)."""
    rows = [np.mean(np.load(p), axis=0) for p in npy_paths]
    out = np.zeros((len(rows),) + rows[0].shape)
    for i, r in enumerate(rows):
        out[i] = r
    return out


def save_mat(path, data_name, matrix):
    import scipy.io
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    scipy.io.savemat(path, {data_name: matrix})
    return path
