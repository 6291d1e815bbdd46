"""The greyscale screen on the MI355X (csrc/greyscale.hip through relax_greyscale_scan / relax_yuv_greyscale_scan and
data_processing.check_greyscale.scan_yuv_file), one session on one card, device events, median of 7 samples with their min and max:

  - the BGR scan of 64 frames at 960x540, 1920x1080 and 3840x2160: ms per call and the share of the 6.29 TB/s device copy rate
    this project measures, for the 3 bytes per pixel it must read.  Each size runs over a ring of buffers that together pass the
    256 MiB Infinity Cache (the figure to quote), and on one buffer called back to back (cache-resident where it fits);
  - the fused YUV scan against the unfused pair relax_yuv_to_bgr + relax_greyscale_scan on the same yuv420p frames, the two
    alternated sample by sample: ms per call each, and whether the fused form wins by more than the larger of the two spreads;
  - a whole-file scan of a page-cached synthetic 1920x1080 yuv420p file of all-grey frames: frames/s, and where the time goes
    (file reads into pinned memory, host-to-device copies, the kernel - each timed alone), beside the host numpy path
    (sampling.yuv_frame_bgr + the rule) on a few frames, EXTRAPOLATED to the file.

  python tools/greyscale_bench.py [--frames 64] [--file-frames 120] [--out profiles/greyscale_bench.json]

Synthetic frames: the timings do not depend on the values.  Not measured here: real dataset files, containers, more than one GPU."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import relax_vqa_amd  # noqa: E402,F401
from relax_vqa_amd import _lib, sampling  # noqa: E402
from relax_vqa_amd.data_processing import check_greyscale  # noqa: E402

COPY_RATE = 6.29e12          # bytes/s moved (read + written) by a device-to-device copy, README's measured figure
L3_BYTES = 256 << 20
SIZES = (((540, 960), 20), ((1080, 1920), 8), ((2160, 3840), 2))      # (H, W), calls per sample


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _samples(calls, inner, n=7):
    """calls: functions timed in turn, sample by sample (alternated) -> one list of ms per call for each."""
    for f in calls:
        for _ in range(2):
            f(0)
    torch.cuda.synchronize()
    ms = [[] for _ in calls]
    for s in range(n):
        for k, f in enumerate(calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(inner):
                f(s * inner + i)
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / inner)
    return ms


def _stats(ms, must_move):
    med = float(np.median(ms))
    return {"ms_per_call_median": med, "ms_per_call_min": min(ms), "ms_per_call_max": max(ms), "spread_ms": max(ms) - min(ms),
            "bytes_that_must_move": must_move, "ms_at_copy_rate": must_move / COPY_RATE * 1e3,
            "frac_of_copy_rate": must_move / COPY_RATE * 1e3 / med, "tb_per_s": must_move / med / 1e9}


def bgr_scan(H, W, frames, inner):
    lib = _lib.load()
    slot = H * W * 3
    ring = max(2, -(-(L3_BYTES * 5 // 4) // (frames * slot)) + 1)
    bufs = [torch.randint(0, 256, (frames * slot,), dtype=torch.uint8, device="cuda") for _ in range(ring)]
    out = torch.empty((frames, 8), dtype=torch.int32, device="cuda")

    def call(buf):
        rc = lib.relax_greyscale_scan(_ptr(buf), slot, frames, H, W, _ptr(out), _stream())
        assert rc == 0, lib.relax_last_error(None).decode()
    past, same = _samples([lambda i: call(bufs[i % ring]), lambda i: call(bufs[0])], inner)
    want = check_greyscale.host_records(bufs[0][:slot].cpu().numpy().reshape(1, H, W, 3))
    call(bufs[0])
    assert np.array_equal(out[:1].cpu().numpy(), want)
    rec = {"frames": frames, "calls_per_sample": inner, "ring_buffers": ring, "ring_mb": ring * frames * slot / 1e6,
           "ring_past_the_infinity_cache": _stats(past, frames * slot), "one_buffer_back_to_back": _stats(same, frames * slot),
           "one_buffer_mb": frames * slot / 1e6}
    return rec


def fused_against_pair(H, W, frames, inner):
    lib = _lib.load()
    layout = sampling.YUV_420P
    fb = sampling.yuv_frame_bytes(layout, H, W)
    stride = (fb + 15) // 16 * 16
    slot = H * W * 3
    ring = max(2, -(-(L3_BYTES * 5 // 4) // (frames * stride)) + 1)
    srcs = [torch.randint(0, 256, (frames * stride,), dtype=torch.uint8, device="cuda") for _ in range(ring)]
    offsets = (torch.arange(frames, dtype=torch.int64) * stride).cuda()
    items = torch.stack([torch.arange(frames, dtype=torch.int64) * stride, torch.arange(frames, dtype=torch.int64) * slot], dim=1).contiguous().cuda()
    bgr = torch.empty(frames * slot, dtype=torch.uint8, device="cuda")
    status = torch.empty(frames, dtype=torch.int32, device="cuda")
    out_f = torch.empty((frames, 8), dtype=torch.int32, device="cuda")
    out_p = torch.empty((frames, 8), dtype=torch.int32, device="cuda")

    def fused(i):
        s = srcs[i % ring]
        rc = lib.relax_yuv_greyscale_scan(_ptr(s), s.numel(), _ptr(offsets), frames, layout, H, W, 0, 0, _ptr(out_f), _stream())
        assert rc == 0, lib.relax_last_error(None).decode()

    def pair(i):
        s = srcs[i % ring]
        rc = lib.relax_yuv_to_bgr(_ptr(s), s.numel(), _ptr(items), frames, layout, H, W, 0, 0, _ptr(bgr), bgr.numel(), _ptr(status), _stream())
        assert rc == 0, lib.relax_last_error(None).decode()
        rc = lib.relax_greyscale_scan(_ptr(bgr), slot, frames, H, W, _ptr(out_p), _stream())
        assert rc == 0, lib.relax_last_error(None).decode()
    f_ms, p_ms = _samples([fused, pair], inner)
    fused(0), pair(0)
    torch.cuda.synchronize()
    assert torch.equal(out_f, out_p)
    f, p = _stats(f_ms, frames * fb), _stats(p_ms, frames * (fb + 2 * slot))
    gain = p["ms_per_call_median"] - f["ms_per_call_median"]
    return {"frames": frames, "calls_per_sample": inner, "ring_buffers": ring, "fused": f, "unfused_pair": p, "records_equal": True,
            "pair_minus_fused_ms": gain, "larger_spread_ms": max(f["spread_ms"], p["spread_ms"]),
            "fused_wins_by_more_than_the_spread": bool(gain > max(f["spread_ms"], p["spread_ms"]))}


def whole_file(directory, n_frames, host_frames=3):
    H, W, pixfmt = 1080, 1920, "yuv420p"
    layout = sampling.YUV_420P
    fb = sampling.yuv_frame_bytes(layout, H, W)
    path = os.path.join(directory, "grey_1080p.yuv")
    rng = np.random.default_rng(1)
    with open(path, "wb") as f:
        for _ in range(n_frames):
            frame = np.full(fb, 128, np.uint8)
            frame[:H * W] = rng.integers(0, 256, H * W, dtype=np.uint8)
            f.write(frame.tobytes())
    res = check_greyscale.scan_yuv_file(path, W, H, pixfmt)                  # warm-up: page cache, pinned buffers, code objects
    assert res["first_colour_frame"] is None and res["frames_scanned"] == n_frames
    runs = [check_greyscale.scan_yuv_file(path, W, H, pixfmt) for _ in range(7)]
    fps = [n_frames / r["seconds"] for r in runs]
    chunk = runs[0]["chunk_frames"]
    slot = (fb + 15) // 16 * 16
    # the three parts, each alone, for one chunk
    pinned = torch.empty(chunk * slot, dtype=torch.uint8, pin_memory=True)
    t_read = []
    for _ in range(7):
        t0 = time.perf_counter()
        sampling.read_yuv_frames(path, list(range(chunk)), fb, slot, pinned.numpy())
        t_read.append((time.perf_counter() - t0) * 1e3)
    dev = torch.empty(chunk * slot, dtype=torch.uint8, device="cuda")
    offsets = (torch.arange(chunk, dtype=torch.int64) * slot).cuda()
    out = torch.empty((chunk, 8), dtype=torch.int32, device="cuda")
    lib = _lib.load()

    def kernel(i):
        rc = lib.relax_yuv_greyscale_scan(_ptr(dev), dev.numel(), _ptr(offsets), chunk, layout, H, W, 0, 0, _ptr(out), _stream())
        assert rc == 0, lib.relax_last_error(None).decode()
    t_copy, t_kernel = _samples([lambda i: dev.copy_(pinned, non_blocking=True), kernel], 1)
    # the host path on a few frames, extrapolated
    t0 = time.perf_counter()
    frames = sampling.load_frames_from_yuv(path, W, H, pixfmt, list(range(host_frames)))
    grey = check_greyscale.records_are_greyscale(check_greyscale.host_records(frames))
    host_s = (time.perf_counter() - t0) / host_frames
    assert bool(grey.all())
    os.remove(path)
    chunks = -(-n_frames // chunk)
    return {"file": f"{n_frames} frames {W}x{H} {pixfmt}, all grey, page-cached", "file_mb": n_frames * fb / 1e6, "chunk_frames": chunk,
            "chunks": chunks, "frames_per_s_median": float(np.median(fps)), "frames_per_s_min": min(fps), "frames_per_s_max": max(fps),
            "seconds_median": float(np.median([r["seconds"] for r in runs])),
            "read_seconds_inside_the_pass_median": float(np.median([r["read_seconds"] for r in runs])),
            "one_chunk_alone_ms": {"read_into_pinned_median": float(np.median(t_read)), "read_min": min(t_read), "read_max": max(t_read),
                                   "h2d_copy_median": float(np.median(t_copy)), "h2d_min": min(t_copy), "h2d_max": max(t_copy),
                                   "kernel_median": float(np.median(t_kernel)), "kernel_min": min(t_kernel), "kernel_max": max(t_kernel)},
            "host_numpy_path": {"frames_timed": host_frames, "seconds_per_frame": host_s,
                                "frames_per_s_EXTRAPOLATED_from_these_frames": 1.0 / host_s,
                                "seconds_for_the_file_EXTRAPOLATED": host_s * n_frames}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--file-frames", type=int, default=120)
    ap.add_argument("--dir", default=None, help="where the synthetic video goes (default: a temporary directory)")
    ap.add_argument("--skip-file", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("greyscale_bench needs the GPU: nothing is measured without one")
    torch.zeros(1, device="cuda")
    rec = {"what": "greyscale screen: relax_greyscale_scan, relax_yuv_greyscale_scan against yuv_to_bgr + scan, scan_yuv_file",
           "device": torch.cuda.get_device_name(0), "copy_rate_bytes_per_s": COPY_RATE, "bgr_scan": {}, "fused_yuv_scan": {}}
    for (H, W), inner in SIZES:
        rec["bgr_scan"][f"{W}x{H}"] = r = bgr_scan(H, W, args.frames, inner)
        q, o = r["ring_past_the_infinity_cache"], r["one_buffer_back_to_back"]
        print(f"bgr {W}x{H}: ring {q['ms_per_call_median']:.4f} ms [{q['ms_per_call_min']:.4f}, {q['ms_per_call_max']:.4f}] "
              f"{100 * q['frac_of_copy_rate']:.0f} % of the copy rate; one buffer {o['ms_per_call_median']:.4f} ms", flush=True)
    for (H, W), inner in SIZES:
        rec["fused_yuv_scan"][f"{W}x{H}"] = r = fused_against_pair(H, W, args.frames, inner)
        print(f"yuv {W}x{H}: fused {r['fused']['ms_per_call_median']:.4f} ms [{r['fused']['ms_per_call_min']:.4f}, "
              f"{r['fused']['ms_per_call_max']:.4f}], pair {r['unfused_pair']['ms_per_call_median']:.4f} ms "
              f"[{r['unfused_pair']['ms_per_call_min']:.4f}, {r['unfused_pair']['ms_per_call_max']:.4f}]", flush=True)
    if not args.skip_file:
        tmp = args.dir or tempfile.mkdtemp(prefix="grey_bench_")
        rec["whole_file"] = w = whole_file(tmp, args.file_frames)
        print(json.dumps(w), flush=True)
    rec["not_measured"] = ["real dataset files", "containers (no decoder in this project)", "more than one GPU"]
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
