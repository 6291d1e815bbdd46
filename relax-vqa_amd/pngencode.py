"""GPU PNG encode (csrc/png_encode.hip through relax_png_encode): uint8 device images -> PNG files, what cv2.imwrite leaves
behind in the reference's drivers (BGR written as RGB, one channel as gray).  All images of a call go through one encode
call (bands of all images in one launch); only the compressed bytes cross to the host, where png.build adds the container
and its CRCs.  Geometry the kernel refuses (channels other than 1 or 3, rows over 16 KiB) is written by Pillow - per file,
counted in `stats`, never an error - as the decoder counts its fallbacks.

A PngEncoder owns a HIP stream, its scratch and output buffers and its pinned landing buffer, and is used by one thread at a
time: encoder_for(device) keeps one per (thread, device), so writer threads encode at the same time, each on its own stream."""
import ctypes as C
import threading

import numpy as np
import torch

from . import _lib, png

COLOR_TYPE = {1: 0, 3: 2}
SINGLE_COPY_BYTES = 32 << 20     # output ranges up to this size are fetched in one copy, slack between the streams included


class PngEncodeError(RuntimeError):
    """An image the encoder refused (the status word names why)."""


def as_items(images):
    """images: a uint8 [N,H,W,3] / [N,H,W] tensor or a list of [H,W,3] / [H,W] tensors (sizes may differ) -> list of
    per-image tensors [H,W,C] or [H,W].  A 3-d tensor whose last dimension is 3 is ONE BGR image [H,W,3]: a gray batch that is
    three pixels wide ([N,H,3]) cannot be told from it and must be passed as a list of [H,3] images."""
    if isinstance(images, torch.Tensor):
        if images.dim() == 4 or (images.dim() == 3 and images.shape[-1] != 3):
            return list(images.unbind(0))
        if images.dim() in (2, 3):
            return [images]
        raise ValueError(f"images must be [N,H,W,3] or [N,H,W], got {tuple(images.shape)}")
    return list(images)


class PngEncoder:
    def __init__(self, device=None):
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.lib = _lib.load()
        self.stream = torch.cuda.Stream(self.device)
        self._pinned = self._scratch = self._out = None
        self.encoded = 0        # images encoded on the GPU, cumulative
        self.fallbacks = 0      # images written by Pillow instead, cumulative

    def _buffer(self, name, n, pinned=False):
        buf = getattr(self, name)
        if buf is None or buf.numel() < n:
            size = max(n, 1 << 16) * 5 // 4
            buf = (torch.empty(size, dtype=torch.uint8, pin_memory=True) if pinned
                   else torch.empty(size, dtype=torch.uint8, device=self.device))
            setattr(self, name, buf)
        return buf

    def geometry(self, H, W, Cc, filt=-1):
        """-> (stream bound, scratch bytes, rows per band) of relax_png_encode_bound, or None if the kernel refuses it."""
        scratch, rows = C.c_int64(0), C.c_int(0)
        b = self.lib.relax_png_encode_bound(H, W, Cc, filt, C.byref(scratch), C.byref(rows))
        return None if b < 0 else (int(b), int(scratch.value), int(rows.value))

    def _prepare(self, img):
        if not isinstance(img, torch.Tensor):
            img = torch.as_tensor(np.asarray(img))
        if img.dtype != torch.uint8 or img.dim() not in (2, 3):
            raise ValueError(f"an image must be uint8 [H,W,3] or [H,W], got {img.dtype} {tuple(img.shape)}")
        if img.device != self.device:
            img = img.to(self.device)
        Cc = 1 if img.dim() == 2 else img.shape[2]
        H, W = img.shape[0], img.shape[1]
        packed = img.stride(1) == Cc and (Cc == 1 or img.stride(2) == 1) and (H == 1 or img.stride(0) >= W * Cc)
        if img.dim() == 3 and Cc == 1:
            packed = packed and img.stride(1) == 1
        return (img if packed else img.contiguous()), H, W, Cc

    def encode_streams(self, images, filter=None, statuses=None, stats=None, scratch_fill=None):
        """-> [(zlib stream bytes | None, H, W, C, image tensor)]: None where the kernel does not take the geometry.
        filter: None (chosen per row), 0..4, or one such value per image.  statuses: a list -> receives one RELAX_PNG_* code
        per image and no error is raised.  scratch_fill: a byte the scratch is filled with first (tests: its contents on
        entry must not matter)."""
        imgs = [self._prepare(im) for im in as_items(images)]
        N = len(imgs)
        filters = [(-1 if filter is None else int(filter))] * N if not isinstance(filter, (list, tuple)) else \
            [(-1 if f is None else int(f)) for f in filter]
        if len(filters) != N:
            raise ValueError("one filter per image")
        geo = [self.geometry(H, W, Cc, f) for (_, H, W, Cc), f in zip(imgs, filters)]
        gpu = [n for n in range(N) if geo[n] is not None]
        result = [(None, H, W, Cc, t) for (t, H, W, Cc) in imgs]
        codes = [0] * N
        if gpu:
            caller = torch.cuda.current_stream(self.device)
            lo = min(imgs[n][0].data_ptr() for n in gpu)
            hi = max(imgs[n][0].data_ptr() + (imgs[n][1] - 1) * (imgs[n][0].stride(0) if imgs[n][1] > 1 else 0) +
                     imgs[n][2] * imgs[n][3] for n in gpu)
            items = np.zeros((len(gpu), 8), np.int64)
            at = scratch_bytes = 0
            for k, n in enumerate(gpu):
                t, H, W, Cc = imgs[n]
                bound, scratch, _ = geo[n]
                items[k] = (t.data_ptr() - lo, t.stride(0) if H > 1 else W * Cc, H, W, Cc, at, bound, filters[n])
                at += (bound + 7) // 8 * 8
                scratch_bytes += scratch
            with torch.cuda.stream(self.stream):
                self.stream.wait_stream(caller)             # the images: whatever the caller queued before
                out = self._buffer("_out", at)
                scratch = self._buffer("_scratch", scratch_bytes)
                if scratch_fill is not None:
                    scratch.fill_(scratch_fill)
                dev_items = torch.from_numpy(items).to(self.device, non_blocking=True)
                lengths = torch.empty(len(gpu), dtype=torch.int64, device=self.device)
                status = torch.empty(len(gpu), dtype=torch.int32, device=self.device)
                rc = self.lib.relax_png_encode(C.c_void_p(lo), hi - lo, C.c_void_p(dev_items.data_ptr()), len(gpu),
                                               C.c_void_p(out.data_ptr()), at, C.c_void_p(scratch.data_ptr()), scratch.numel(),
                                               C.c_void_p(lengths.data_ptr()), C.c_void_p(status.data_ptr()),
                                               C.c_void_p(self.stream.cuda_stream))
                if rc != 0:
                    raise RuntimeError(f"relax_png_encode failed ({rc}): {self.lib.relax_last_error(None).decode()}")
                for n in gpu:
                    imgs[n][0].record_stream(self.stream)
                lens = lengths.cpu().tolist()               # waits for the encode
                st = status.cpu().tolist()
                # Only the streams cross to the host.  Small slots (fragments) go in ONE copy of the whole output range - the bound
                # is tight enough that this costs less than a copy per image; large ones are copied stream by stream.
                whole = at <= SINGLE_COPY_BYTES
                starts = []
                if whole:
                    pinned = self._buffer("_pinned", at, pinned=True)
                    pinned[:at].copy_(out[:at], non_blocking=True)
                    starts = [int(items[k, 5]) for k in range(len(gpu))]
                else:
                    pinned = self._buffer("_pinned", int(sum(lens)), pinned=True)
                    pos = 0
                    for k in range(len(gpu)):
                        starts.append(pos)
                        if lens[k]:
                            o = int(items[k, 5])
                            pinned[pos:pos + lens[k]].copy_(out[o:o + lens[k]], non_blocking=True)
                            pos += lens[k]
                self.stream.synchronize()
            host = pinned.numpy()
            for k, n in enumerate(gpu):
                codes[n] = st[k]
                if st[k] == 0:
                    t, H, W, Cc = imgs[n]
                    result[n] = (host[starts[k]:starts[k] + lens[k]].tobytes(), H, W, Cc, t)
        self.encoded += len(gpu)
        self.fallbacks += N - len(gpu)
        if stats is not None:
            stats["gpu"] = stats.get("gpu", 0) + len(gpu)
            stats["fallback"] = stats.get("fallback", 0) + N - len(gpu)
        if statuses is not None:
            statuses.extend(codes)
        else:
            for n, c in enumerate(codes):
                if c:
                    raise PngEncodeError(f"image {n}: PNG encode failed: {png.status_message(c)} (status {c})")
        return result

    def encode(self, images, filter=None, stats=None):
        """-> list of bytes, one PNG file per image."""
        files = []
        for z, H, W, Cc, t in self.encode_streams(images, filter=filter, stats=stats):
            files.append(png.build(z, W, H, COLOR_TYPE[Cc]) if z is not None else _pillow_png(t))
        return files

    def write(self, paths, images, filter=None, stats=None):
        """One file per image, as cv2.imwrite(path, image) writes it (equal on the decoded pixels)."""
        items = as_items(images)
        paths = [paths] if isinstance(paths, (str, bytes)) or hasattr(paths, "__fspath__") else list(paths)
        if len(paths) != len(items):
            raise ValueError(f"{len(paths)} paths for {len(items)} images")
        for path, data in zip(paths, self.encode(items, filter=filter, stats=stats)):
            with open(path, "wb") as f:
                f.write(data)


def _pillow_png(t):
    """The host path for geometry the kernel refuses: BGR(A) -> RGB(A), gray as it is."""
    import io

    from PIL import Image
    a = t.cpu().numpy()
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[..., 0]
    if a.ndim == 3:
        if a.shape[2] not in (3, 4):
            raise ValueError(f"cannot write an image with {a.shape[2]} channels")
        a = a[..., [2, 1, 0] + ([3] if a.shape[2] == 4 else [])]
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(a)).save(buf, format="PNG", compress_level=1)
    return buf.getvalue()


_tls = threading.local()


def encoder_for(device=None):
    """This thread's encoder for `device` (created on first use)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    per = getattr(_tls, "encoders", None)
    if per is None:
        per = _tls.encoders = {}
    e = per.get(dev.index)
    if e is None:
        e = per[dev.index] = PngEncoder(dev)
    return e
