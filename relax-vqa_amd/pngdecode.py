"""GPU PNG decode (csrc/png_decode.hip through relax_png_decode): files or bytes -> uint8 BGR device tensors, equal to
sampling.read_frame_bgr (cv2.imread).  The container is parsed on the host (png.py); the zlib streams go to the device in one
copy and one launch decodes them all, one workgroup per image.  Files the GPU path does not take (16-bit, palette, gray + alpha,
Adam7) are decoded on the host with read_frame_bgr and uploaded into the same tensor - per file, counted, never an error.

A PngDecoder owns a HIP stream, its scratch and its pinned staging buffer, and is used by one thread at a time:
decoder_for(device) keeps one per (thread, device), so loader threads decode at the same time, each on its own stream."""
import ctypes as C
import threading

import numpy as np
import torch

from . import _lib, png


class PngDecodeError(RuntimeError):
    """A file whose image data the decoder refused (the status word names why)."""


class PngDecoder:
    def __init__(self, device=None):
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.lib = _lib.load()
        self.stream = torch.cuda.Stream(self.device)
        self._pinned = None
        self._raw = None
        self.decoded = 0        # images decoded on the GPU, cumulative
        self.fallbacks = 0      # files decoded on the host instead, cumulative

    def _pinned_bytes(self, n):
        if self._pinned is None or self._pinned.numel() < n:
            self._pinned = torch.empty(max(n, 1 << 20) * 5 // 4, dtype=torch.uint8, pin_memory=True)
        return self._pinned

    def decode(self, sources, out=None, statuses=None, stats=None, consumer=None, parsed=None):
        """sources: file paths or bytes.  -> uint8 BGR on the device: [N,H,W,3] if every image has one size, else a list of
        [H,W,3] tensors; or `out` (a uint8 [N,H,W,3] view with contiguous rows, e.g. clip.view(-1,H,W,3)) filled.
        statuses: a list -> receives one RELAX_PNG_* code per source (0 for host fallbacks) and no error is raised for a bad
        stream; otherwise the first bad stream raises PngDecodeError naming the file and the status.  stats: a dict -> gets
        'gpu' and 'fallback' counts of this call.  consumer: the stream that will read the result (default: the caller's
        current stream); the tensor is recorded on it, so the caching allocator does not hand its memory out again while
        that stream may still read it.  Returns after the decode stream has finished."""
        if parsed is None:
            parsed = []
            for s in sources:
                name, data = png.read_source(s)
                parsed.append((name, png.parse(data, name)))
        N = len(parsed)
        caller = torch.cuda.current_stream(self.device)
        consumer = caller if consumer is None else consumer
        shapes = [info.shape for _, info in parsed]
        same = N > 0 and all(s == shapes[0] for s in shapes)
        if out is not None:
            if out.dtype != torch.uint8 or out.device != self.device or out.dim() != 4 or out.shape[0] != N:
                raise ValueError(f"out must be uint8 [N={N},H,W,3] on {self.device}, got {out.dtype} {tuple(out.shape)} on {out.device}")
            for (name, info) in parsed:
                if tuple(out.shape[1:]) != info.shape:
                    raise ValueError(f"{name}: image {info.shape} does not fit out {tuple(out.shape[1:])}")
            Hh, Ww = out.shape[1], out.shape[2]
            if out.stride()[1:] != (Ww * 3, 3, 1) or (N > 1 and out.stride(0) < Hh * Ww * 3):
                raise ValueError(f"out must hold each image as contiguous rows in its own slot, strides {out.stride()}")
            offsets = [n * out.stride(0) for n in range(N)]
        else:
            sizes = [h * w * 3 for h, w, _ in shapes]
            offsets = list(np.cumsum([0] + sizes[:-1])) if N else []
        gpu = [n for n, (_, info) in enumerate(parsed) if info.channels is not None]
        host = [n for n in range(N) if parsed[n][1].channels is None]
        # staging: the zlib streams, then the item table (8-aligned), in one pinned buffer -> one host-to-device copy
        zlens = [len(parsed[n][1].zdata) for n in gpu]
        zbytes = int(sum(zlens))
        items_at = (zbytes + 7) // 8 * 8
        total = items_at + 64 * len(gpu)
        pinned = self._pinned_bytes(total)
        host_view = pinned.numpy()
        items = np.zeros((len(gpu), 8), np.int64)
        at = raw_at = 0
        for k, n in enumerate(gpu):
            info = parsed[n][1]
            zl = zlens[k]
            host_view[at:at + zl] = np.frombuffer(info.zdata, np.uint8)
            items[k] = (at, zl, raw_at, offsets[n], info.height, info.width, info.channels, 0)
            at += zl
            raw_at += info.height * (1 + info.width * info.channels)
        host_view[items_at:total] = items.view(np.uint8).reshape(-1)
        with torch.cuda.stream(self.stream):
            self.stream.wait_stream(caller)                 # `out` and reused memory: whatever the caller queued before
            if out is None:
                flat = torch.empty(int(sum(h * w * 3 for h, w, _ in shapes)), dtype=torch.uint8, device=self.device)
                base, out_bytes = flat, flat.numel()
            else:
                base, out_bytes = out, (N - 1) * out.stride(0) + out.shape[1] * out.shape[2] * 3 if N else 0
            status = torch.zeros(len(gpu), dtype=torch.int32, device=self.device)
            if gpu:
                dev = pinned[:total].to(self.device, non_blocking=True)
                if self._raw is None or self._raw.numel() < raw_at:
                    self._raw = torch.empty(raw_at * 5 // 4, dtype=torch.uint8, device=self.device)
                rc = self.lib.relax_png_decode(C.c_void_p(dev.data_ptr()), zbytes, C.c_void_p(dev.data_ptr() + items_at), len(gpu),
                                               C.c_void_p(base.data_ptr()), out_bytes, C.c_void_p(self._raw.data_ptr()),
                                               self._raw.numel(), C.c_void_p(status.data_ptr()),
                                               C.c_void_p(self.stream.cuda_stream))
                if rc != 0:
                    raise RuntimeError(f"relax_png_decode failed ({rc}): {self.lib.relax_last_error(None).decode()}")
            for n in host:                                  # host fallback, under the GPU decode
                from . import sampling
                img = torch.from_numpy(sampling.read_frame_bgr(parsed[n][0]) if parsed[n][0] != "<bytes>"
                                       else _pillow_bgr(sources[n]))
                dst = base.view(-1)[offsets[n]:offsets[n] + img.numel()] if out is None else out[n]
                dst.copy_(img.view(dst.shape))
            st = status.cpu()                               # waits for the decode
            self.stream.synchronize()
        self.decoded += len(gpu)
        self.fallbacks += len(host)
        if stats is not None:
            stats["gpu"] = stats.get("gpu", 0) + len(gpu)
            stats["fallback"] = stats.get("fallback", 0) + len(host)
        codes = [0] * N
        for k, n in enumerate(gpu):
            codes[n] = int(st[k])
        if statuses is not None:
            statuses.extend(codes)
        else:
            for n, c in enumerate(codes):
                if c:
                    raise PngDecodeError(f"{parsed[n][0]}: PNG decode failed: {png.status_message(c)} (status {c})")
        if out is None:
            base.record_stream(consumer)
            if same:
                h, w, _ = shapes[0]
                return base.view(N, h, w, 3)
            return [base[o:o + h * w * 3].view(h, w, 3) for o, (h, w, _) in zip(offsets, shapes)]
        return out


def _pillow_bgr(data):
    import io

    from PIL import Image
    with Image.open(io.BytesIO(bytes(data))) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[..., ::-1])


_tls = threading.local()


def decoder_for(device=None):
    """This thread's decoder for `device` (created on first use)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    per = getattr(_tls, "decoders", None)
    if per is None:
        per = _tls.decoders = {}
    d = per.get(dev.index)
    if d is None:
        d = per[dev.index] = PngDecoder(dev)
    return d
