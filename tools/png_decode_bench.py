"""GPU PNG decode on the MI355X (csrc/png_decode.hip through RelaxEngine.decode_png / sampling.GpuFrameLoader):

  - decodes/s at 960x540 and 1920x1080 of three kinds of file, each with the same content as bench.py's from-files frames
    (bench.write_frame_files: low-pass noise + fine noise):
      pillow  - as bench.py writes them (Pillow, compress_level=3, adaptive filters: Sub, Up and Paeth mixed)
      ffmpeg  - as ffmpeg writes them (filter None on every row, zlib level 6, 4 KiB IDAT chunks)
      paeth   - every row Paeth (the un-filter's serial worst case), zlib level 6
    'batch' = one decode_png call of --batch files from one thread (file read + container parse + upload + kernel),
    'kernel' = the same batch with the containers parsed beforehand, 'threads' = --threads loader threads decoding batches at
    the same time, each on its own stream (aggregate rate);
  - a from-files config-4 dataset pass (1024 clips of 16 pairs at 960x540) with GpuFrameLoader in the loader threads, beside
    the same pass over device-resident clips, both in this process.

  python tools/png_decode_bench.py [--batch 64] [--reps 5] [--threads 8] [--clips 1024] [--out profiles/png_decode_bench.json]

Synthetic weights (synth.*_state_dict): the timing does not depend on the values."""
import argparse
import json
import os
import struct
import sys
import tempfile
import threading
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import relax_vqa_amd  # noqa: E402,F401
from relax_vqa_amd import dataset, png, pngdecode, sampling, synth  # noqa: E402
from relax_vqa_amd.engine import RelaxEngine  # noqa: E402


def _chunk(ctype, body):
    return struct.pack(">I", len(body)) + ctype + body + struct.pack(">I", zlib.crc32(body, zlib.crc32(ctype)))


def _paeth_rows(rows):
    """RGB rows uint8 [H, W*3] -> the filtered stream with filter 4 (Paeth) on every row."""
    H, n = rows.shape
    out = []
    prev = np.zeros(n, np.int32)
    for y in range(H):
        x = rows[y].astype(np.int32)
        a = np.concatenate([np.zeros(3, np.int32), x[:-3]])
        c = np.concatenate([np.zeros(3, np.int32), prev[:-3]])
        p = a + prev - c
        pa, pb, pc = np.abs(p - a), np.abs(p - prev), np.abs(p - c)
        pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, prev, c))
        out.append(b"\x04" + ((x - pred) & 255).astype(np.uint8).tobytes())
        prev = x
    return b"".join(out)


def write_png(path, rgb, kind):
    H, W, _ = rgb.shape
    rows = rgb.reshape(H, W * 3)
    raw = _paeth_rows(rows) if kind == "paeth" else b"".join(b"\x00" + r.tobytes() for r in rows)
    z = zlib.compress(raw, 6)
    body = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))
    body += b"".join(_chunk(b"IDAT", z[i:i + 4096]) for i in range(0, len(z), 4096))
    with open(path, "wb") as f:
        f.write(body + _chunk(b"IEND", b""))


def make_files(directory, H, W, n):
    """n frames of each kind at H x W -> {kind: [paths]} (the pillow kind is bench.write_frame_files itself)."""
    import bench
    from PIL import Image
    d = os.path.join(directory, f"{W}x{H}")
    names = bench.write_frame_files(d, 1, n // 2, H, W)
    pillow = [p for t in range(n // 2) for p in (os.path.join(d, f"{names[0]}_{t}.png"), os.path.join(d, f"{names[0]}_{t}_next.png"))]
    out = {"pillow": pillow, "ffmpeg": [], "paeth": []}
    for k, p in enumerate(pillow):
        rgb = np.asarray(Image.open(p).convert("RGB"))
        for kind in ("ffmpeg", "paeth"):
            q = os.path.join(d, f"{kind}_{k}.png")
            if not os.path.exists(q):
                write_png(q, rgb, kind)
            out[kind].append(q)
    return out


def rate(fn, n_images, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return n_images / float(np.median(ts))


def decode_rates(paths, batch, reps, threads):
    order = [paths[i % len(paths)] for i in range(batch)]
    dec = pngdecode.decoder_for(0)
    parsed = []
    for p in order:
        name, data = png.read_source(p)
        parsed.append((name, png.parse(data, name)))
    info = parsed[0][1]
    out = torch.empty((batch, info.height, info.width, 3), dtype=torch.uint8, device="cuda")
    r_batch = rate(lambda: dec.decode(order, out=out), batch, reps)
    r_kernel = rate(lambda: dec.decode(None, out=out, parsed=parsed), batch, reps)

    def many():
        def work():
            d = pngdecode.decoder_for(0)
            o = torch.empty_like(out)
            for _ in range(2):
                d.decode(order, out=o)
        ts = [threading.Thread(target=work) for _ in range(threads)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
    r_threads = rate(many, batch * 2 * threads, max(2, reps // 2))
    mb = float(np.mean([os.path.getsize(p) for p in paths])) / 1e6
    return {"batch_decodes_per_s": r_batch, "kernel_decodes_per_s": r_kernel, "threads_decodes_per_s": r_threads,
            "file_mb": mb, "zlib_ratio": info.height * (1 + info.width * 3) / len(info.zdata)}


def dataset_rates(eng, directory, n_clips, workers_list):
    H, W, T = 540, 960, 16
    d = os.path.join(directory, "config4")
    import bench
    names = bench.write_frame_files(d, 4, T, H, W)
    resident = [torch.from_numpy(synth.synthetic_clip(T, H, W, clip_id=700 + i, distinct=4)).cuda() for i in range(4)]
    kw = dict(clips_per_step=64, resnet=True, vit=True, rank=0, world=1)
    out = {}

    def timed(source, workers):
        dataset.extract_dataset_clips(source, 64, eng, workers=workers, ramp=False, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m, errors = dataset.extract_dataset_clips(source, n_clips, eng, workers=workers, **kw)
        torch.cuda.synchronize()
        assert not errors and bool(torch.isfinite(m).all()), errors[:3]
        return n_clips / (time.perf_counter() - t0), m

    out["device_resident_clips_per_s"], _ = timed(lambda i: resident[i % 4], 8)
    loader = sampling.GpuFrameLoader(d, [names[i % 4] for i in range(n_clips)], device=eng.device)
    out["gpu_loader"] = []
    for w in workers_list:
        r, _ = timed(loader, w)
        out["gpu_loader"].append({"loader_threads": w, "clips_per_s": r, "png_decodes_per_s": r * 2 * T,
                                  "frac_of_device_resident": r / out["device_resident_clips_per_s"]})
    # the frame files are not the resident clips' pixels: the GPU loader's rows are checked against the Pillow loader's
    pil, e = dataset.extract_dataset_clips(lambda i: sampling.load_clip_from_frames(d, names[i % 4]), 8, eng, workers=8, **kw)
    gpu, e2 = dataset.extract_dataset_clips(loader, 8, eng, workers=8, **kw)
    out["matrix_equal_to_pillow_loader"] = bool(not e and not e2 and torch.equal(pil, gpu))
    out["fallbacks"] = loader.fallbacks
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--workers", default="8,16")
    ap.add_argument("--dir", default=None, help="where the frame files go (default: a temporary directory)")
    ap.add_argument("--skip-dataset", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    eng = RelaxEngine(0)
    tmp = args.dir or tempfile.mkdtemp(prefix="png_bench_")
    rec = {"what": "GPU PNG decode (relax_png_decode), uint8 BGR equal to cv2.imread; decodes/s include reading the file from "
                   "the page cache, the container parse and the upload unless marked kernel",
           "batch": args.batch, "threads": args.threads, "decode": {}}
    for H, W in ((540, 960), (1080, 1920)):
        files = make_files(tmp, H, W, 16)
        for kind, paths in files.items():
            r = decode_rates(paths, args.batch, args.reps, args.threads)
            rec["decode"][f"{W}x{H}_{kind}"] = r
            print(f"{W}x{H} {kind:7s} {r['file_mb']:.2f} MB ratio {r['zlib_ratio']:.1f}: batch {r['batch_decodes_per_s']:.0f}/s "
                  f"kernel {r['kernel_decodes_per_s']:.0f}/s {args.threads} threads {r['threads_decodes_per_s']:.0f}/s", flush=True)
    if not args.skip_dataset:
        rn, vt = synth.resnet50_state_dict(), synth.vit_state_dict("vit_base")
        eng.load_resnet50(rn)
        eng.load_vit(vt, "vit_base")
        ds = dataset_rates(eng, tmp, args.clips, [int(w) for w in args.workers.split(",")])
        ds["pillow_loader_threads_clips_per_s"] = 30.1      # profiles/r06_from_files_config4.json (16 loader threads)
        rec["dataset_config4_from_files"] = ds
        print(json.dumps(ds), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
