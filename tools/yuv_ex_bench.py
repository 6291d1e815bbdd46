"""The RELAX_YUVF_* formats on the MI355X (csrc/yuv.hip: relax_yuv_to_bgr_ex; csrc/greyscale.hip: relax_yuv_greyscale_scan_ex), one
session on one card, the kernels alone:

  - every format at 1920x1080 and 3840x2160, 64 frames per call on the 16-byte path: ms per call from device events (each sample
    times --inner back-to-back calls that walk a ring of source and output buffers larger than the 256 MiB Infinity Cache, so no
    call finds its frames or its slots cached; median of 7 samples with their min and max), the bytes that must move (frame bytes
    in, 3 per pixel out), TB/s and the share of the 6.29 TB/s device copy rate this project measures;
  - yuv420p through relax_yuv_to_bgr_ex against relax_yuv_to_bgr, alternated sample by sample (the `_ex` entry launches the same
    kernel: the two must lie within each other's spread);
  - for yuv420p10le and uyvy422 the fused relax_yuv_greyscale_scan_ex against relax_yuv_to_bgr_ex + relax_greyscale_scan,
    alternated sample by sample: the fused form stays for a format only if it wins by more than the larger of the two spreads.

  python tools/yuv_ex_bench.py [--out profiles/yuv_ex_bench.json]

Random bytes: the timings do not depend on the values.  Not measured here: real dataset files, ffmpeg's own output, file reads and
host-to-device copies (tools/yuv_ingest_bench.py measures those for yuv420p), more than one GPU."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import relax_vqa_amd  # noqa: E402,F401
from relax_vqa_amd import _lib, sampling  # noqa: E402

COPY_RATE = 6.29e12          # bytes/s moved (read + written) by a device-to-device copy, README's measured figure
CACHE = 256 << 20            # Infinity Cache
FRAMES = 64
SAMPLES = 7
SIZES = (((1080, 1920), 10), ((2160, 3840), 4))      # (H, W), calls per sample


def _ptr(t):
    return C.c_void_p(t.data_ptr())


class Ring:
    """`sets` source regions and output regions, each FRAMES frames at 16-byte-aligned slots, inside two big device buffers; together
    past four times the Infinity Cache."""

    def __init__(self, pool_src, pool_out, fb, H, W):
        self.slot_in, self.slot_out = (fb + 15) // 16 * 16, H * W * 3
        set_bytes = FRAMES * (self.slot_in + self.slot_out)
        self.sets = max(2, -(-4 * CACHE // set_bytes))
        assert self.sets * FRAMES * self.slot_in <= pool_src.numel() and self.sets * FRAMES * self.slot_out <= pool_out.numel()
        self.src, self.out = pool_src, pool_out
        k = torch.arange(self.sets * FRAMES, dtype=torch.int64)
        self.items = torch.stack([k * self.slot_in, k * self.slot_out], dim=1).contiguous().cuda()      # [sets * FRAMES, 2]
        self.offsets = (k * self.slot_in).cuda()
        self.status = torch.empty(self.sets * FRAMES, dtype=torch.int32, device="cuda")
        self.records = torch.empty((self.sets * FRAMES, 8), dtype=torch.int32, device="cuda")
        self.turn = 0

    def next(self):
        s = self.turn % self.sets
        self.turn += 1
        return s


def _samples(fns, inner):
    """Device-event ms per call of each function, SAMPLES samples of `inner` calls each, the functions alternated sample by sample."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(SAMPLES):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b) / inner)
    return ms


def _row(ms, moved, inner):
    med = float(np.median(ms))
    return {"ms_per_call_median": med, "ms_per_call_min": min(ms), "ms_per_call_max": max(ms), "calls_per_sample": inner, "samples": len(ms),
            "bytes_moved": moved, "tb_per_s": moved / med / 1e9, "frac_of_copy_rate": moved / COPY_RATE * 1e3 / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("yuv_ex_bench needs the GPU: nothing is measured without one")
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    names = list(sampling._YUV_FORMATS)
    names = [n for n in names if not n.startswith("yuvj")]
    Hm, Wm = SIZES[-1][0]
    worst_fb = max(sampling.yuv_frame_bytes_ex(sampling.yuv_format(n)[0], Hm, Wm) for n in names)
    pool_src = torch.randint(0, 256, (2 * FRAMES * (worst_fb + 16),), dtype=torch.uint8, device="cuda")
    pool_out = torch.empty(2 * FRAMES * Hm * Wm * 3 + (4 * CACHE), dtype=torch.uint8, device="cuda")
    rec = {"what": "relax_yuv_to_bgr_ex / relax_yuv_greyscale_scan_ex per format: kernels alone from device events, 64 frames per call, "
                   "a ring of buffers past the Infinity Cache, median of 7 samples [min, max], one session, one card",
           "device": torch.cuda.get_device_name(0), "copy_rate_bytes_per_s": COPY_RATE, "frames_per_call": FRAMES, "convert": {},
           "ex_entry_against_old_entry_yuv420p": {}, "fused_scan_against_pair": {},
           "not_measured": "real dataset files, ffmpeg's own output, file reads and host-to-device copies, more than one GPU"}

    def convert(entry, fmt, H, W, ring):
        def fn():
            s = ring.next() * FRAMES
            rc = entry(_ptr(ring.src), ring.src.numel(), _ptr(ring.items[s]), FRAMES, fmt, H, W, 0, 0, _ptr(ring.out), ring.out.numel(),
                       _ptr(ring.status[s]), stream)
            assert rc == 0, lib.relax_last_error(None).decode()
        return fn

    def fused(fmt, H, W, ring):
        def fn():
            s = ring.next() * FRAMES
            rc = lib.relax_yuv_greyscale_scan_ex(_ptr(ring.src), ring.src.numel(), _ptr(ring.offsets[s]), FRAMES, fmt, H, W, 0, 0,
                                                 _ptr(ring.records[s]), stream)
            assert rc == 0, lib.relax_last_error(None).decode()
        return fn

    def pair(fmt, H, W, ring):
        to_bgr = convert(lib.relax_yuv_to_bgr_ex, fmt, H, W, ring)

        def fn():
            s = (ring.turn % ring.sets) * FRAMES
            to_bgr()
            rc = lib.relax_greyscale_scan(C.c_void_p(ring.out.data_ptr() + s * ring.slot_out), ring.slot_out, FRAMES, H, W,
                                          _ptr(ring.records[s]), stream)
            assert rc == 0, lib.relax_last_error(None).decode()
        return fn

    for (H, W), inner in SIZES:
        size = f"{W}x{H}"
        for name in names:
            fmt, _ = sampling.yuv_format(name)
            fb = sampling.yuv_frame_bytes_ex(fmt, H, W)
            ring = Ring(pool_src, pool_out, fb, H, W)
            ms, = _samples([convert(lib.relax_yuv_to_bgr_ex, fmt, H, W, ring)], inner)
            assert not bool(ring.status.any())
            rec["convert"].setdefault(size, {})[name] = r = _row(ms, FRAMES * (fb + H * W * 3), inner)
            r["ring_sets"], r["ring_mb"] = ring.sets, ring.sets * FRAMES * (ring.slot_in + ring.slot_out) / 1e6
            print(f"{size} {name}: {r['ms_per_call_median']:.4f} ms [{r['ms_per_call_min']:.4f}, {r['ms_per_call_max']:.4f}] "
                  f"{r['tb_per_s']:.2f} TB/s, {100 * r['frac_of_copy_rate']:.0f} % of the copy rate", flush=True)
        fb = sampling.yuv_frame_bytes(0, H, W)
        ring = Ring(pool_src, pool_out, fb, H, W)
        old, new = _samples([convert(lib.relax_yuv_to_bgr, 0, H, W, ring), convert(lib.relax_yuv_to_bgr_ex, 0, H, W, ring)], inner)
        moved = FRAMES * (fb + H * W * 3)
        rec["ex_entry_against_old_entry_yuv420p"][size] = r = {"relax_yuv_to_bgr": _row(old, moved, inner), "relax_yuv_to_bgr_ex": _row(new, moved, inner)}
        lo = max(min(old), min(new))
        r["within_spread"] = bool(lo <= min(max(old), max(new)))              # the two [min, max] ranges overlap
        print(f"{size} yuv420p old entry {np.median(old):.4f} [{min(old):.4f}, {max(old):.4f}]  _ex {np.median(new):.4f} "
              f"[{min(new):.4f}, {max(new):.4f}]  within spread: {r['within_spread']}", flush=True)
        for name in ("yuv420p10le", "uyvy422"):
            fmt, _ = sampling.yuv_format(name)
            fb = sampling.yuv_frame_bytes_ex(fmt, H, W)
            ring = Ring(pool_src, pool_out, fb, H, W)
            f_ms, p_ms = _samples([fused(fmt, H, W, ring), pair(fmt, H, W, ring)], inner)
            spread = max(max(f_ms) - min(f_ms), max(p_ms) - min(p_ms))
            rec["fused_scan_against_pair"].setdefault(size, {})[name] = r = {
                "fused": _row(f_ms, FRAMES * fb, inner), "pair": _row(p_ms, FRAMES * (fb + 2 * H * W * 3), inner), "larger_spread_ms": spread,
                "fused_wins_by_ms": float(np.median(p_ms) - np.median(f_ms)),
                "fused_kept": bool(np.median(p_ms) - np.median(f_ms) > spread)}
            print(f"{size} {name}: fused {np.median(f_ms):.4f} ms, pair {np.median(p_ms):.4f} ms, larger spread {spread:.4f} ms, "
                  f"fused kept: {r['fused_kept']}", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
