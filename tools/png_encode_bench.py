"""Times the GPU PNG encoder (relax_png_encode) and the path it replaces, and writes profiles/png_encode_bench.json.
Workloads: 64 fragments of 224 x 224 and 32 frames at 540p, 1080p and 2160p, each on the committed golden frames (tiled or
cropped) and on noise.  Device events, median of 7: the whole encode call; the encode launches alone (plan + bands) and the
compaction alone (placement + copy, on the scratch the encode launches left: relax_png_encode_passes); the device-to-host
copy of the compressed bytes.  Wall clock, median of 7: host CRC + container (png.build) and the whole
RelaxEngine-level encode after a warm-up call.  The path a user has without the encoder (the raw frame copied to the host,
then Pillow's Image.save at compress_level 1) and Pillow's sizes at levels 1 and 6 are measured on the first 4 images, one
pass; the replaced path's time for the batch is EXTRAPOLATED from them (x N / 4) and named so.  Reported, not gated.

    python tools/png_encode_bench.py [--out profiles/png_encode_bench.json] [--quick]"""
import argparse
import ctypes as C
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import relax_vqa_amd  # noqa: E402,F401
from relax_vqa_amd import png, pngencode  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def golden(stem, suffix=""):
    from PIL import Image
    with Image.open(os.path.join(GOLDEN, "png_" + stem, f"{stem}{suffix}.png")) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[..., ::-1])


def tiled(frame, H, W):
    reps = (-(-H // frame.shape[0]), -(-W // frame.shape[1]), 1)
    return np.ascontiguousarray(np.tile(frame, reps)[:H, :W])


def events_ms(fn, reps=7):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def run(name, batch, enc):
    """batch uint8 [N,H,W,3] on the device."""
    from PIL import Image
    N, H, W, _ = batch.shape
    lib = enc.lib
    bound, scratch_one, rows = enc.geometry(H, W, 3)
    slot = (bound + 7) // 8 * 8
    items = np.zeros((N, 8), np.int64)
    for n in range(N):
        items[n] = (n * H * W * 3, W * 3, H, W, 3, n * slot, bound, -1)
    dev = batch.device
    d_items = torch.from_numpy(items).to(dev)
    out = torch.empty(N * slot, dtype=torch.uint8, device=dev)
    scratch = torch.empty(N * scratch_one, dtype=torch.uint8, device=dev)
    lengths = torch.empty(N, dtype=torch.int64, device=dev)
    status = torch.empty(N, dtype=torch.int32, device=dev)

    def encode():
        rc = lib.relax_png_encode(C.c_void_p(batch.data_ptr()), batch.numel(), C.c_void_p(d_items.data_ptr()), N,
                                  C.c_void_p(out.data_ptr()), out.numel(), C.c_void_p(scratch.data_ptr()), scratch.numel(),
                                  C.c_void_p(lengths.data_ptr()), C.c_void_p(status.data_ptr()),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0

    def passes(which):
        def fn():
            rc = lib.relax_png_encode_passes(C.c_void_p(batch.data_ptr()), batch.numel(), C.c_void_p(d_items.data_ptr()), N,
                                             C.c_void_p(out.data_ptr()), out.numel(), C.c_void_p(scratch.data_ptr()),
                                             scratch.numel(), C.c_void_p(lengths.data_ptr()), C.c_void_p(status.data_ptr()), which,
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0
        return fn

    encode_ms = events_ms(encode)
    bands_ms = events_ms(passes(1 | 2))             # plan + bands
    compact_ms = events_ms(passes(4 | 8))           # placement + copy, on the scratch the line above left
    assert int(status.abs().sum()) == 0
    lens = lengths.cpu().tolist()
    total = int(sum(lens))
    pinned = torch.empty(total, dtype=torch.uint8, pin_memory=True)

    def copy_out():
        pos = 0
        for n in range(N):
            pinned[pos:pos + lens[n]].copy_(out[n * slot:n * slot + lens[n]], non_blocking=True)
            pos += lens[n]

    copy_ms = events_ms(copy_out)
    host = pinned.numpy()
    walls = []
    for _ in range(7):
        t0 = time.perf_counter()
        pos = 0
        files = []
        for n in range(N):
            files.append(png.build(host[pos:pos + lens[n]].tobytes(), W, H, 2))
            pos += lens[n]
        walls.append((time.perf_counter() - t0) * 1e3)
    container_ms = statistics.median(walls)
    with Image.open(io.BytesIO(files[0])) as im:
        assert np.array_equal(np.asarray(im)[..., ::-1], batch[0].cpu().numpy())
    assert enc.encode(batch) == files                # warm-up: the encoder's buffers are allocated here
    walls = []
    for _ in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        enc.encode(batch)
        walls.append((time.perf_counter() - t0) * 1e3)
    end_to_end_ms = statistics.median(walls)
    # the path it replaces, and Pillow's sizes, over the first k images
    k = min(N, 4)
    sizes = {}
    t0 = time.perf_counter()
    for n in range(k):
        a = batch[n].cpu().numpy()[..., ::-1]
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(a)).save(buf, format="PNG", compress_level=1)
        sizes.setdefault(1, []).append(buf.tell())
    pillow_ms = (time.perf_counter() - t0) * 1e3 / k * N
    for n in range(k):
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(batch[n].cpu().numpy()[..., ::-1])).save(buf, format="PNG", compress_level=6)
        sizes.setdefault(6, []).append(buf.tell())
    raw = N * H * W * 3
    return dict(workload=name, images=N, height=H, width=W, band_rows=rows, raw_bytes=raw,
                encode_call_ms=round(encode_ms, 4), encode_GBps_raw=round(raw / encode_ms / 1e6, 2),
                encode_launches_plan_and_bands_ms=round(bands_ms, 4), compaction_place_and_copy_ms=round(compact_ms, 4),
                copy_compressed_to_host_ms=round(copy_ms, 4), host_crc_and_container_ms=round(container_ms, 3),
                encode_png_end_to_end_wall_ms=round(end_to_end_ms, 3),
                replaced_path_copy_plus_pillow_level1_wall_ms_extrapolated=round(pillow_ms, 1), replaced_path_measured_on_images=k,
                bytes_per_image=round(total / N), pillow_level1_bytes_per_image=round(sum(sizes[1]) / k),
                pillow_level6_bytes_per_image=round(sum(sizes[6]) / k), compressed_over_raw=round(total / raw, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_encode_bench.json"))
    ap.add_argument("--quick", action="store_true", help="fragments and 540p only")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    enc = pngencode.PngEncoder(dev)
    frag = golden("TelevisionClip_1080P-68c6_1", "_ori_frag")
    tv, small = golden("TelevisionClip_1080P-68c6_1"), golden("5636101558_3")
    rng = np.random.default_rng(0)
    plans = [("fragments_224", 64, 224, 224, frag), ("frames_540p", 32, 540, 960, small)]
    if not args.quick:
        plans += [("frames_1080p", 32, 1080, 1920, tv), ("frames_2160p", 32, 2160, 3840, tv)]
    results = []
    for name, N, H, W, src in plans:
        base = tiled(src, H, W)
        frames = np.stack([np.roll(base, 7 * n, axis=1) for n in range(N)])
        for kind, data in (("golden", frames), ("noise", None)):
            if data is None:
                batch = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device=dev, generator=torch.Generator(dev).manual_seed(1))
            else:
                batch = torch.from_numpy(data).to(dev)
            r = run(f"{name}_{kind}", batch, enc)
            print(json.dumps(r), flush=True)
            results.append(r)
            del batch
            torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), method="device events, median of 7; wall-clock figures: median of 7; the replaced path: one pass over 4 images, scaled to the batch",
                       results=results), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
