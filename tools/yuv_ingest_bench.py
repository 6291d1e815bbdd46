"""Raw YUV ingest on the MI355X (csrc/yuv.hip through relax_yuv_to_bgr / sampling.GpuYuvLoader), one session on one card:

  - the kernel alone on T = 32 pairs (64 yuv420p frames, one launch) at 960x540, 1920x1080 and 3840x2160: ms per call from device
    events (each sample times --inner back-to-back calls; median of 7 samples with their min and max), the bytes it moves (1.5 in +
    3 out per pixel) and the time those bytes take at the 6.29 TB/s device copy rate this project measures; the 16-byte path, and
    at 960x540 the bytewise path too (every frame one byte off alignment);
  - a config-4-shaped from-files dataset pass (clips of 16 pairs at 960x540) over synthetic .yuv files (framerate 30: the sampled
    frames lie 15 apart, each read with its successor) with GpuYuvLoader in the loader threads, against the same clips through
    load_clip_from_yuv (host conversion into the pinned pool, the `alloc` protocol) and through load_clip_from_frames on PNG files
    of the same frames (the path a from-files pass takes today), beside the pass over device-resident clips - all in this process.

  python tools/yuv_ingest_bench.py [--clips 1024] [--host-clips 192] [--workers 16] [--out profiles/yuv_ingest_bench.json]

Synthetic weights and frames: the timings do not depend on the values.  Not measured here: real LIVE-Qualcomm files, ffmpeg's own
output, more than one GPU."""
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
from relax_vqa_amd import _lib, dataset, sampling, synth  # noqa: E402
from relax_vqa_amd.engine import RelaxEngine  # noqa: E402

COPY_RATE = 6.29e12          # bytes/s moved (read + written) by a device-to-device copy, README's measured figure


def kernel_times(H, W, pairs, inner, misalign=0):
    lib = _lib.load()
    layout = sampling.YUV_420P
    fb = sampling.yuv_frame_bytes(layout, H, W)
    n = 2 * pairs
    stride = (fb + 15) // 16 * 16
    src = torch.randint(0, 256, (n * stride + 16,), dtype=torch.uint8, device="cuda")
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
    items = torch.tensor([(k * stride + misalign, k * H * W * 3) for k in range(n)], dtype=torch.int64).cuda()
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream()

    def call():
        rc = lib.relax_yuv_to_bgr(C.c_void_p(src.data_ptr()), src.numel(), C.c_void_p(items.data_ptr()), n, layout, H, W, 0, 0,
                                  C.c_void_p(out.data_ptr()), out.numel(), C.c_void_p(status.data_ptr()), C.c_void_p(stream.cuda_stream))
        assert rc == 0, lib.relax_last_error(None).decode()
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    assert not bool(status.any())
    ms = []
    for _ in range(7):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    moved = n * (fb + H * W * 3)
    med = float(np.median(ms))
    return {"frames": n, "ms_per_call_median": med, "ms_per_call_min": min(ms), "ms_per_call_max": max(ms), "calls_per_sample": inner,
            "bytes_moved": moved, "ms_at_copy_rate": moved / COPY_RATE * 1e3, "frac_of_copy_rate": moved / COPY_RATE * 1e3 / med,
            "tb_per_s": moved / med / 1e9, "working_set_mb": moved / 1e6}


def make_videos(directory, n_videos, T, H, W, framerate):
    """n_videos raw yuv420p files whose sampled frames and successors carry synthetic content (the frames in between are never
    read and stay holes), and PNG files of the same frames as the reference's ffmpeg step names them."""
    from PIL import Image
    os.makedirs(directory, exist_ok=True)
    k = sampling.frame_interval(framerate)
    n_frames = k * (T - 1) + 2
    fb = sampling.yuv_frame_bytes(sampling.YUV_420P, H, W)
    paths, names = [], []
    for v in range(n_videos):
        bgr = synth.synthetic_clip(T, H, W, clip_id=900 + v, distinct=4)       # [T,2,H,W,3]: its channels serve as Y, U, V planes
        p = os.path.join(directory, f"video{v}.yuv")
        with open(p, "wb") as f:
            f.truncate(n_frames * fb)
            for t in range(T):
                for j in (0, 1):
                    img = bgr[t, j]
                    frame = np.concatenate([img[..., 1].reshape(-1), img[::2, ::2, 0].reshape(-1), img[::2, ::2, 2].reshape(-1)])
                    f.seek((t * k + j) * fb)
                    f.write(frame.tobytes())
        clip = sampling.load_clip_from_yuv(p, W, H, "yuv420p", framerate)
        assert clip.shape[0] == T
        d = os.path.join(directory, f"frames{v}")
        os.makedirs(d, exist_ok=True)
        for t in range(T):
            Image.fromarray(clip[t, 0][..., ::-1]).save(os.path.join(d, f"video{v}_{t * k}.png"), compress_level=3)
            Image.fromarray(clip[t, 1][..., ::-1]).save(os.path.join(d, f"video{v}_{t * k}_next.png"), compress_level=3)
        paths.append(p)
        names.append((d, f"video{v}"))
    return paths, names


def dataset_rates(eng, directory, n_clips, host_clips, workers, repeats):
    H, W, T, framerate, V = 540, 960, 16, 30, 4
    paths, names = make_videos(directory, V, T, H, W, framerate)
    resident = [torch.from_numpy(sampling.load_clip_from_yuv(p, W, H, "yuv420p", framerate)).cuda() for p in paths]
    kw = dict(clips_per_step=64, resnet=True, vit=True, rank=0, world=1)
    loader = sampling.GpuYuvLoader([paths[i % V] for i in range(n_clips)], W, H, "yuv420p", framerate, device=eng.device)

    def host_yuv(i, alloc=None):
        return sampling.load_clip_from_yuv(paths[i % V], W, H, "yuv420p", framerate, alloc=alloc)

    def host_png(i, alloc=None):
        d, name = names[i % V]
        return sampling.load_clip_from_frames(d, name, alloc=alloc)
    sources = {"device_resident": (lambda i: resident[i % V], n_clips), "gpu_yuv_loader": (loader, n_clips),
               "host_yuv_loader": (host_yuv, host_clips), "png_files_pillow": (host_png, host_clips)}
    out = {"clips": {k: n for k, (_, n) in sources.items()}, "loader_threads": workers, "pairs_per_clip": T, "frame": f"{W}x{H}",
           "framerate": framerate, "yuv_bytes_read_per_clip": 2 * T * sampling.yuv_frame_bytes(0, H, W),
           "png_bytes_read_per_clip": sum(os.path.getsize(os.path.join(names[0][0], f)) for f in os.listdir(names[0][0]))}
    rows = {}
    for name, (src, n) in sources.items():
        dataset.extract_dataset_clips(src, 64, eng, workers=workers, ramp=False, **kw)      # warm-up: code objects, pinned pool, page cache
        torch.cuda.synchronize()
    rates = {name: [] for name in sources}
    for _ in range(repeats):                                                                  # alternate the sources: same session, same card
        for name, (src, n) in sources.items():
            timings = {}
            t0 = time.perf_counter()
            m, errors = dataset.extract_dataset_clips(src, n, eng, workers=workers, timings=timings, **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert not errors and bool(torch.isfinite(m).all()), errors[:3]
            rates[name].append(n / dt)
            rows[name] = m[:V].clone()
            out.setdefault("loader_wait_s", {})[name] = timings.get("loader_wait_s")
    for name, r in rates.items():
        out[name] = {"clips_per_s_median": float(np.median(r)), "clips_per_s_min": min(r), "clips_per_s_max": max(r), "runs": len(r)}
    out["rows_equal_across_sources"] = bool(all(torch.equal(rows["device_resident"], rows[k]) for k in rows))
    # where one GpuYuvLoader call spends its time, one thread, nothing else running: read (page cache -> pinned), copy + kernel
    one = sampling.GpuYuvLoader([paths[0]], W, H, "yuv420p", framerate, device=eng.device)
    one(0)
    t0 = time.perf_counter()
    for _ in range(20):
        one(0)
    out["gpu_yuv_loader_one_thread_ms_per_clip"] = (time.perf_counter() - t0) / 20 * 1e3
    fb = sampling.yuv_frame_bytes(0, H, W)
    buf = np.empty(2 * fb, np.uint8)
    fd = os.open(paths[0], os.O_RDONLY)
    t0 = time.perf_counter()
    for _ in range(20):
        for t in range(T):
            os.preadv(fd, [memoryview(buf)], t * sampling.frame_interval(framerate) * fb)
    out["read_alone_ms_per_clip"] = (time.perf_counter() - t0) / 20 * 1e3
    os.close(fd)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--host-clips", type=int, default=192)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--dir", default=None, help="where the video and frame files go (default: a temporary directory)")
    ap.add_argument("--skip-dataset", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("yuv_ingest_bench needs the GPU: nothing is measured without one")
    eng = RelaxEngine(0)
    rec = {"what": "raw yuv420p -> BGR (relax_yuv_to_bgr): kernel alone from device events, and from-files config-4 dataset passes",
           "device": torch.cuda.get_device_name(0), "copy_rate_bytes_per_s": COPY_RATE, "kernel": {}}
    for (H, W), inner in (((540, 960), 50), ((1080, 1920), 20), ((2160, 3840), 5)):
        rec["kernel"][f"{W}x{H}_fast"] = r = kernel_times(H, W, args.pairs, inner)
        print(f"{W}x{H} 16-byte path: {r['ms_per_call_median']:.4f} ms [{r['ms_per_call_min']:.4f}, {r['ms_per_call_max']:.4f}] "
              f"{r['tb_per_s']:.2f} TB/s, {100 * r['frac_of_copy_rate']:.0f} % of the copy rate", flush=True)
    rec["kernel"]["960x540_bytewise"] = r = kernel_times(540, 960, args.pairs, 10, misalign=1)
    print(f"960x540 bytewise: {r['ms_per_call_median']:.4f} ms [{r['ms_per_call_min']:.4f}, {r['ms_per_call_max']:.4f}] {r['tb_per_s']:.2f} TB/s",
          flush=True)
    rec["kernel_note"] = ("the 960x540 working set (149 MB) fits the 256 MiB Infinity Cache and is re-read by the back-to-back calls; "
                          "1080p (597 MB) and 2160p (2.4 GB) do not fit")
    if not args.skip_dataset:
        eng.load_resnet50(synth.resnet50_state_dict())
        eng.load_vit(synth.vit_state_dict("vit_base"), "vit_base")
        tmp = args.dir or tempfile.mkdtemp(prefix="yuv_bench_")
        rec["dataset_config4_from_files"] = ds = dataset_rates(eng, tmp, args.clips, args.host_clips, args.workers, args.repeats)
        print(json.dumps(ds), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
