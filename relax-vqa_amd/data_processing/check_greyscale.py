"""The greyscale screen of the reference's src/data_processing/check_greyscale.py, on the GPU.

The reference drops every video its greyscale reports list before it splits, fine-tunes or recovers a median model
(split_train_test.py:15-21,49-50, fine_tune.py:72-75,94, recover_median_train_test.py:23-27,50).  The reports come from this
screen: a video is greyscale iff every frame is, and a BGR frame is greyscale iff

    max(b - g) <= 3 and max(b - r) <= 3 and max(g - r) <= 3        (is_greyscale_image, :25-35)

with b, g, r uint8 numpy views, so each difference wraps modulo 256 before cv2.norm takes its maximum: b - g = -1 is 255 and the
frame counts as colour.  That is mode='reference', the default, because the committed reports were made with it; mode='abs'
compares |b - g|, |b - r|, |g - r|.  One scan gives the maxima of both (include/relax_hip.h: relax_greyscale_scan for BGR
frames, relax_yuv_greyscale_scan straight from raw YUV frames), so a caller re-thresholds without a second pass.

  is_greyscale_image        <- is_greyscale_image (:25-35)
  check_video_greyscale     <- check_video_greyscale (:37-55), for raw .yuv files and directories of PNG frames
  scan_yuv_file             the whole-file pass behind it: chunked reads, two pinned buffers, early stop
  process_videos_from_csv   <- process_videos_from_csv (:57-95): the report `Index,vid,Is Greyscale`
  greyscale_indices         <- `pd.read_csv(report).iloc[:, 0].tolist()` of the scripts that apply a report
"""
import csv
import ctypes as C
import os
import time

import numpy as np

from .. import sampling, video_frames_extract

RECORD_WORDS = 8                     # RELAX_GREYSCALE_RECORD_WORDS
MODES = {"reference": 0, "abs": 3}   # first of the three maxima of a record
STAGING_BYTES = 64 << 20             # each of scan_yuv_file's two pinned buffers, at most (one frame at least)
REPORT_COLUMNS = ("Index", "vid", "Is Greyscale")
RAW_SUFFIXES = (".yuv",)


def _mode(mode):
    if mode not in MODES:
        raise ValueError(f"mode {mode!r} is not one of {', '.join(MODES)}")
    return MODES[mode]


def records_are_greyscale(records, threshold=3, mode="reference"):
    """Records [N,8] (numpy or torch) -> bool [N]: all three maxima of `mode` <= threshold."""
    lo = _mode(mode)
    return (records[..., lo:lo + 3] <= threshold).all(-1)


class GreyscaleScan(dict):
    """What a scan returns: 'records' int32 [N,8] and its views 'wrapped' [N,3] (maxima of (b-g, b-r, g-r) mod 256), 'abs'
    [N,3] (maxima of |b-g|, |b-r|, |g-r|) and 'status' [N] - device tensors - plus is_greyscale()."""

    def __init__(self, records):
        super().__init__(records=records, wrapped=records[:, 0:3], abs=records[:, 3:6], status=records[:, 6])

    def is_greyscale(self, threshold=3, mode="reference"):
        return records_are_greyscale(self["records"], threshold, mode)


def host_records(frames):
    """The numpy statement of a record, from the rule above: uint8 [N,H,W,3] -> int32 [N,8]."""
    frames = np.asarray(frames)
    if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[-1] != 3:
        raise ValueError(f"expected uint8 [N,H,W,3], got {frames.dtype} {frames.shape}")
    out = np.zeros((frames.shape[0], RECORD_WORDS), np.int32)
    b, g, r = (frames[..., c].reshape(frames.shape[0], -1) for c in range(3))
    for q, (x, y) in enumerate(((b, g), (b, r), (g, r))):
        if x.shape[1]:
            out[:, q] = (x - y).max(axis=1)                                   # uint8 arithmetic: wraps modulo 256
            out[:, 3 + q] = np.abs(x.astype(np.int16) - y.astype(np.int16)).max(axis=1)
    return out


def _stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def scan_frames(frames):
    """uint8 device frames -> GreyscaleScan.  frames: [N,H,W,3], [T,2,H,W,3] (N = 2T, in storage order), a strided view of
    either whose frames keep packed rows, or [N,H,W] - single-channel frames are greyscale by the reference's first branch: zero
    records, nothing launched.  Runs on the current stream of the frames' device."""
    import torch

    from .. import _lib
    if not isinstance(frames, torch.Tensor) or not frames.is_cuda or frames.dtype != torch.uint8:
        raise TypeError("scan_frames: expected a uint8 device tensor")
    if frames.dim() == 3:
        return GreyscaleScan(torch.zeros((frames.shape[0], RECORD_WORDS), dtype=torch.int32, device=frames.device))
    if frames.dim() == 5:
        if frames.shape[1] != 2:
            raise ValueError(f"scan_frames: a clip is [T,2,H,W,3], got {tuple(frames.shape)}")
        if frames.shape[0] > 1 and frames.stride(0) != 2 * frames.stride(1):
            frames = frames.contiguous()
        frames = frames.as_strided((2 * frames.shape[0],) + tuple(frames.shape[2:]), (frames.stride(1),) + tuple(frames.stride()[2:]))
    if frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError(f"scan_frames: expected [N,H,W,3], [T,2,H,W,3] or [N,H,W], got {tuple(frames.shape)}")
    N, H, W, _ = frames.shape
    if N == 0 or H == 0 or W == 0:
        raise ValueError(f"scan_frames: empty frames {tuple(frames.shape)}")
    if frames.stride()[1:] != (W * 3, 3, 1) or (N > 1 and frames.stride(0) < H * W * 3):
        raise ValueError(f"scan_frames: every frame must hold packed rows in its own slot, strides {frames.stride()}")
    lib = _lib.load()
    with torch.cuda.device(frames.device):
        records = torch.empty((N, RECORD_WORDS), dtype=torch.int32, device=frames.device)
        rc = lib.relax_greyscale_scan(C.c_void_p(frames.data_ptr()), frames.stride(0) if N > 1 else H * W * 3, N, H, W,
                                      C.c_void_p(records.data_ptr()), _stream_ptr())
    if rc != 0:
        raise RuntimeError(f"relax_greyscale_scan failed ({rc}): {lib.relax_last_error(None).decode()}")
    return GreyscaleScan(records)


def _yuv_scan_entry(lib, extended):
    return (lib.relax_yuv_greyscale_scan_ex, "relax_yuv_greyscale_scan_ex") if extended else (lib.relax_yuv_greyscale_scan, "relax_yuv_greyscale_scan")


def scan_yuv_frames(planes, H, W, pixfmt, matrix="bt601", offsets=None, out=None, extended=False):
    """Raw 8-bit YUV frames on the device -> GreyscaleScan, without writing BGR (relax_yuv_greyscale_scan): frame by frame the
    records of scan_frames(engine.yuv_to_bgr(...)).  planes: uint8 device tensor holding N whole frames back to back, or any
    bytes with `offsets` (int64 [N], host or device: where each frame starts).  out: an int32 [N,8] device tensor to fill.
    extended=True: pixfmt is one of sampling.yuv_format's names (10 / 12-bit, packed 4:2:2, 4:1:1, 4:1:0, NV21 too) and the scan is
    relax_yuv_greyscale_scan_ex."""
    import torch

    from .. import _lib
    layout, full_range, frame_bytes, _ = sampling._yuv_source(pixfmt, extended)
    if matrix not in sampling.YUV_MATRICES:
        raise ValueError(f"matrix {matrix!r} is not one of {', '.join(sampling.YUV_MATRICES)}")
    H, W = int(H), int(W)
    fb = frame_bytes(H, W)
    if not isinstance(planes, torch.Tensor) or not planes.is_cuda or planes.dtype != torch.uint8:
        raise TypeError("scan_yuv_frames: expected a uint8 device tensor")
    src = planes.contiguous().view(-1)
    if offsets is None:
        if src.numel() % fb:
            raise ValueError(f"{src.numel()} bytes is not a whole number of {W}x{H} {pixfmt} frames of {fb} bytes")
        offsets = torch.arange(src.numel() // fb, dtype=torch.int64, device=src.device) * fb    # on the device: no host copy to wait for
    offsets = torch.as_tensor(offsets, dtype=torch.int64).reshape(-1).to(src.device).contiguous()
    N = offsets.numel()
    lib = _lib.load()
    scan, name = _yuv_scan_entry(lib, extended)
    with torch.cuda.device(src.device):
        if out is None:
            out = torch.empty((N, RECORD_WORDS), dtype=torch.int32, device=src.device)
        elif out.dtype != torch.int32 or tuple(out.shape) != (N, RECORD_WORDS) or not out.is_contiguous() or out.device != src.device:
            raise ValueError(f"out must be a contiguous int32 [{N},{RECORD_WORDS}] tensor on {src.device}")
        rc = scan(C.c_void_p(src.data_ptr()), src.numel(), C.c_void_p(offsets.data_ptr()), N, layout, H, W,
                  sampling.YUV_MATRICES[matrix], int(full_range), C.c_void_p(out.data_ptr()), _stream_ptr())
    if rc != 0:
        raise RuntimeError(f"{name} failed ({rc}): {lib.relax_last_error(None).decode()}")
    return GreyscaleScan(out)


def is_greyscale_image(image, threshold=3, mode="reference"):
    """is_greyscale_image (:25-35): [H,W] -> True; uint8 [H,W,3] BGR -> the rule; anything else False, as the reference's
    fall-through.  A host array is judged on the host, a device tensor by scan_frames."""
    _mode(mode)
    if len(image.shape) == 2:
        return True
    if len(image.shape) != 3 or image.shape[2] != 3:
        return False
    if isinstance(image, np.ndarray) or not getattr(image, "is_cuda", False):
        return bool(records_are_greyscale(host_records(np.asarray(image)[None]), threshold, mode)[0])
    return bool(scan_frames(image.unsqueeze(0)).is_greyscale(threshold, mode)[0])


def scan_yuv_file(video_path, width, height, pixfmt, chunk_frames=None, matrix="bt601", device=None, threshold=3, mode="reference",
                  stop_at_colour=True, extended=False):
    """Every frame of a raw YUV file through relax_yuv_greyscale_scan (extended=True: relax_yuv_greyscale_scan_ex, pixfmt one of
    sampling.yuv_format's names), in file order.

    The frames are read in chunks of `chunk_frames` (default and upper limit: what fits 64 MiB, one frame at least) with
    sampling.read_yuv_frames into one of two pinned staging buffers, every frame at a 16-byte-aligned slot as in GpuYuvLoader;
    a chunk's upload and scan run on a stream of their own while the next chunk is read.  Once a chunk has reported a colour
    frame (under threshold and mode) no further chunk is issued; one more may already be in flight, and it is counted.  With
    stop_at_colour=False the whole file is scanned.

    -> {'first_colour_frame': index or None, 'frames_scanned', 'n_frames', 'records': host int32 [frames_scanned, 8],
        'chunk_frames', 'read_seconds' (host time in the file reads), 'seconds' (the whole pass)}"""
    import torch

    from .. import _lib
    lo = _mode(mode)
    layout, full_range, frame_bytes, _ = sampling._yuv_source(pixfmt, extended)
    if matrix not in sampling.YUV_MATRICES:
        raise ValueError(f"matrix {matrix!r} is not one of {', '.join(sampling.YUV_MATRICES)}")
    H, W = int(height), int(width)
    n = sampling.yuv_frame_count(video_path, W, H, pixfmt, extended)
    fb = frame_bytes(H, W)
    slot = (fb + 15) // 16 * 16
    limit = max(1, STAGING_BYTES // slot)
    chunk = limit if chunk_frames is None else max(1, min(int(chunk_frames), limit))
    chunk = max(1, min(chunk, n))
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    lib = _lib.load()
    scan, name = _yuv_scan_entry(lib, extended)
    t_start = time.perf_counter()
    result = {"first_colour_frame": None, "frames_scanned": 0, "n_frames": n, "chunk_frames": chunk, "read_seconds": 0.0}
    parts = []
    if n:
        stream = torch.cuda.Stream(dev)
        pinned = [torch.empty(chunk * slot, dtype=torch.uint8, pin_memory=True) for _ in range(min(2, -(-n // chunk)))]
        with torch.cuda.stream(stream):
            staged = [torch.empty(chunk * slot, dtype=torch.uint8, device=dev) for _ in pinned]
            offsets = (torch.arange(chunk, dtype=torch.int64) * slot).to(dev)
        pending = None                                             # (first frame, count, device records) of the chunk in flight

        def collect(item):
            first, count, records = item
            with torch.cuda.stream(stream):
                host = records.cpu().numpy()                       # waits for that chunk's scan: its pinned buffer is free again
            parts.append(host)
            result["frames_scanned"] += count
            colour = np.flatnonzero(~(host[:, lo:lo + 3] <= threshold).all(-1))
            if colour.size and result["first_colour_frame"] is None:
                result["first_colour_frame"] = first + int(colour[0])

        for c, first in enumerate(range(0, n, chunk)):
            count = min(chunk, n - first)
            t0 = time.perf_counter()
            sampling.read_yuv_frames(video_path, list(range(first, first + count)), fb, slot, pinned[c % 2].numpy())
            result["read_seconds"] += time.perf_counter() - t0
            with torch.cuda.stream(stream):
                staged[c % 2][:count * slot].copy_(pinned[c % 2][:count * slot], non_blocking=True)
                records = torch.empty((count, RECORD_WORDS), dtype=torch.int32, device=dev)
                rc = scan(C.c_void_p(staged[c % 2].data_ptr()), count * slot, C.c_void_p(offsets.data_ptr()),
                          count, layout, H, W, sampling.YUV_MATRICES[matrix], int(full_range),
                          C.c_void_p(records.data_ptr()), C.c_void_p(stream.cuda_stream))
                if rc != 0:
                    raise RuntimeError(f"{name} failed ({rc}): {lib.relax_last_error(None).decode()}")
            if pending is not None:
                collect(pending)                                   # the chunk before this one; this one is in flight meanwhile
            pending = (first, count, records)
            if stop_at_colour and result["first_colour_frame"] is not None:
                break
        collect(pending)
        stream.synchronize()
    result["records"] = np.concatenate(parts) if parts else np.zeros((0, RECORD_WORDS), np.int32)
    if (result["records"][:, 6] != 0).any():
        raise RuntimeError(f"{video_path}: {name} refused frames {np.flatnonzero(result['records'][:, 6]).tolist()}")
    result["seconds"] = time.perf_counter() - t_start
    return result


def _png_frames(directory):
    return sorted(os.path.join(directory, f) for f in os.listdir(directory) if f.lower().endswith(".png"))


def check_video_greyscale(video_path, width=None, height=None, pixfmt=None, chunk_frames=None, device=None, threshold=3,
                          mode="reference", extended=False):
    """check_video_greyscale (:37-55) -> (is_greyscale, frame_read): (False, True) at the first colour frame, (True, True) if
    every frame passed and at least one was read, (False, False) if no frame could be read - a missing file, a file shorter than
    one frame, a directory without PNG files.

    video_path: a raw .yuv file (width and height as the metadata give them - required, a raw file has no header; pixfmt default
    yuv420p, what the reference assumes for live_qualcomm) scanned by scan_yuv_file; or a directory of PNG frames, decoded on the GPU (pngdecode) in sorted
    order, chunk_frames at a time.  Containers (mp4, mkv, avi, ...) need a demuxer and a decoder and raise NotImplementedError as
    video_frames_extract does: decode them to raw frames or PNGs first.  extended=True: a raw file's pixfmt may be any of
    sampling.yuv_format's names."""
    _mode(mode)
    video_path = os.fspath(video_path)
    if os.path.isdir(video_path):
        paths = _png_frames(video_path)
        if not paths:
            return False, False
        from .. import pngdecode
        step = max(1, int(chunk_frames or 16))
        for k in range(0, len(paths), step):
            frames = pngdecode.decoder_for(device).decode(paths[k:k + step])
            for batch in (frames if isinstance(frames, list) else [frames]):
                batch = batch if batch.dim() == 4 else batch.unsqueeze(0)
                if not bool(scan_frames(batch).is_greyscale(threshold, mode).all()):
                    return False, True
        return True, True
    suffix = os.path.splitext(video_path)[1].lower()
    if suffix not in RAW_SUFFIXES:
        raise video_frames_extract.container_error(suffix.lstrip(".") or "unknown", os.path.basename(video_path))
    if not os.path.isfile(video_path) or os.path.getsize(video_path) == 0:
        return False, False
    if width is None or height is None:
        raise ValueError(f"{video_path}: a raw file has no header - width and height must be given (the metadata's columns)")
    W, H, pixfmt = int(width), int(height), pixfmt or "yuv420p"
    fb = sampling._yuv_source(pixfmt, extended)[2](H, W)
    if os.path.getsize(video_path) < fb:
        return False, False
    res = scan_yuv_file(video_path, W, H, pixfmt, chunk_frames=chunk_frames, device=device, threshold=threshold, mode=mode,
                        extended=extended)
    return res["first_colour_frame"] is None and res["frames_scanned"] > 0, res["frames_scanned"] > 0


# ---- the report ------------------------------------------------------------------------------------------------------------------
def read_report(report_csv):
    """A greyscale report -> [(Index, vid, Is Greyscale)] with Index an int and the flag a bool; the header must be the reference's."""
    with open(report_csv, newline="") as f:
        rows = list(csv.reader(f))
    if not rows or tuple(rows[0]) != REPORT_COLUMNS:
        raise ValueError(f"{report_csv}: header {rows[0] if rows else None} is not {list(REPORT_COLUMNS)}")
    return [(int(r[0]), r[1], r[2].strip() == "True") for r in rows[1:] if r]


def write_report(report_csv, rows):
    """[(Index, vid, Is Greyscale)] -> the file pandas' to_csv(index=False) writes for the reference's result rows."""
    with open(report_csv, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(REPORT_COLUMNS)
        for index, vid, flag in rows:
            w.writerow((int(index), vid, "True" if flag else "False"))


def greyscale_indices(report_csv):
    """The first column of a report as a list of ints: `pd.read_csv(report).iloc[:, 0].tolist()`, the row numbers the reference
    drops from a dataset's metadata and feature matrix (metrics.drop_rows applies them)."""
    return [row[0] for row in read_report(report_csv)]


def video_path_for(data_name, video_dir, row):
    """Where the reference's process_videos_from_csv (:62-73) looks for a row's video, under video_dir: raw .yuv for
    live_qualcomm; otherwise a directory of PNG frames named after the vid if there is one, else the dataset's container file."""
    vid = row["vid"]
    if data_name == "live_qualcomm":
        return os.path.join(video_dir, f"{vid}.yuv")
    frames = os.path.join(video_dir, vid)
    if os.path.isdir(frames):
        return frames
    if data_name == "youtube_ugc":
        return os.path.join(video_dir, f"{row['resolution']}P", f"{vid}.mkv")
    return os.path.join(video_dir, f"{vid}.avi" if data_name == "cvd_2014" else f"{vid}.mp4")


def process_videos_from_csv(metadata_path, output_csv, data_name, video_dir, chunk_frames=None, device=None, threshold=3,
                            mode="reference", extended=False):
    """process_videos_from_csv (:57-95): every row of the metadata file is screened (raw files with the row's width, height and
    pixfmt), and the rows of the greyscale videos alone go to output_csv as `Index,vid,Is Greyscale`, Index being the row number in
    the metadata file (extended: as check_video_greyscale).  No file is written when no video is greyscale.  -> the report rows."""
    with open(metadata_path, newline="") as f:
        meta = list(csv.DictReader(f))
    rows = []
    for i, row in enumerate(meta):
        grey, _ = check_video_greyscale(video_path_for(data_name, video_dir, row), row.get("width"), row.get("height"), row.get("pixfmt"),
                                        chunk_frames=chunk_frames, device=device, threshold=threshold, mode=mode, extended=extended)
        if grey:
            rows.append((i, row["vid"], True))
    if rows:
        write_report(output_csv, rows)
    return rows
