"""Raw YUV frames on the GPU (csrc/yuv.hip: relax_yuv_to_bgr, RelaxEngine.yuv_to_bgr, sampling.GpuYuvLoader) against the numpy
statement of the same integer arithmetic (sampling.yuv_frame_bgr): bit for bit, through the C-ABI."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

from relax_vqa_amd import _lib, dataset, sampling, video_frames_extract
from tests.gpu_common import engine, rn50_weights, vit_weights

pytestmark = pytest.mark.gpu

FILL = 0xA5
SIZES = [(2, 2), (16, 2), (34, 18), (97, 131), (64, 32), (960, 540)]      # W, H
LAYOUTS = {"420p": sampling.YUV_420P, "422p": sampling.YUV_422P, "444p": sampling.YUV_444P, "nv12": sampling.YUV_NV12}


def _convert(src, items, layout, H, W, matrix, full_range, out, out_bytes):
    """relax_yuv_to_bgr on device tensors; -> status words (host)."""
    lib = _lib.load()
    dev_items = torch.tensor(items, dtype=torch.int64).reshape(-1, 2).cuda()
    status = torch.full((len(items),), -7, dtype=torch.int32, device="cuda")
    rc = lib.relax_yuv_to_bgr(C.c_void_p(src.data_ptr()), src.numel(), C.c_void_p(dev_items.data_ptr()), len(items), layout, H, W,
                              sampling.YUV_MATRICES[matrix], int(full_range), C.c_void_p(out.data_ptr()), out_bytes,
                              C.c_void_p(status.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.relax_last_error(None).decode()
    return status.cpu().tolist()


def _host_bgr(frame, layout, H, W, matrix, full_range):
    return sampling.yuv_frame_bgr(*sampling.yuv_planes(frame, layout, H, W), matrix=matrix, full_range=full_range)


@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
@pytest.mark.parametrize("full_range", [False, True], ids=["limited", "full"])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_bit_equal_to_numpy_in_strided_slots(name, full_range, matrix):
    """Three frames back to back in one buffer (frame 1 of 34x18 starts at byte 918: unaligned, the bytewise path; 64x32 and
    960x540 stay on the 16-byte path) and a copy of frame 0 one byte past them (bytewise at every size), written into the
    strided slots of a [T,2,H,W,3] tensor between guard bytes: every slot equals numpy, no other byte changes."""
    layout = LAYOUTS[name]
    rng = np.random.default_rng(17)
    for W, H in SIZES:
        fb = sampling.yuv_frame_bytes(layout, H, W)
        frames = rng.integers(0, 256, (3, fb), dtype=np.uint8)
        src = np.concatenate([frames.reshape(-1), np.zeros(1, np.uint8), frames[0]])
        offsets = [0, fb, 2 * fb, 3 * fb + 1]
        slot, guard, tail = H * W * 3, 64, 256
        buf = torch.full((guard + 4 * (slot + guard) + tail,), FILL, dtype=torch.uint8, device="cuda")
        out = buf[guard:]
        clip = out.as_strided((2, 2, H, W, 3), (2 * (slot + guard), slot + guard, W * 3, 3, 1))
        order = [2, 0, 3, 1]                                                  # item n goes to slot order[n]
        items = [(offsets[n], order[n] * (slot + guard)) for n in range(4)]
        out_bytes = 3 * (slot + guard) + slot                                 # ends with the last slot: its guard and the tail lie past `out`
        status = _convert(torch.from_numpy(src).cuda(), items, layout, H, W, matrix, full_range, out, out_bytes)
        assert status == [0, 0, 0, 0], (W, H)
        host = buf.cpu().numpy()
        mask = np.ones(host.size, bool)
        for n in range(4):
            lo = guard + order[n] * (slot + guard)
            want = _host_bgr(frames[n % 3] if n < 3 else frames[0], layout, H, W, matrix, full_range)
            assert np.array_equal(host[lo:lo + slot].reshape(H, W, 3), want), (W, H, n)
            assert np.array_equal(clip[order[n] // 2, order[n] % 2].cpu().numpy(), want)
            mask[lo:lo + slot] = False
        assert (host[mask] == FILL).all(), (W, H)


_triples = {}


def _all_triples():
    if not _triples:
        y, u, v = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
        _triples["frame"] = np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)])
        _triples["dev"] = torch.from_numpy(_triples["frame"]).cuda()
    return _triples["frame"], _triples["dev"]


@pytest.mark.parametrize("full_range", [False, True], ids=["limited", "full"])
def test_every_triple_in_one_4096_frame(full_range):
    frame, dev = _all_triples()
    got = engine().yuv_to_bgr(dev, 4096, 4096, "yuvj444p" if full_range else "yuv444p")
    want = _host_bgr(frame, sampling.YUV_444P, 4096, 4096, "bt601", full_range)
    assert tuple(got.shape) == (1, 4096, 4096, 3) and np.array_equal(got[0].cpu().numpy(), want)


def test_out_of_range_items_write_nothing_and_spare_the_call():
    W, H, layout = 64, 32, sampling.YUV_420P
    fb, slot, guard = sampling.yuv_frame_bytes(layout, H, W), H * W * 3, 64
    rng = np.random.default_rng(23)
    frames = rng.integers(0, 256, (2, fb), dtype=np.uint8)
    src = torch.from_numpy(frames.reshape(-1)).cuda()
    nslots = 6
    buf = torch.full((guard + nslots * (slot + guard) + 4 * slot,), FILL, dtype=torch.uint8, device="cuda")
    out = buf[guard:]
    out_bytes = (nslots - 1) * (slot + guard) + slot
    step = slot + guard
    items = [(0, 0),
             (2 * fb, 1 * step),                    # source offset past src_bytes
             (fb, 2 * step),
             (fb + 16, 3 * step),                   # the frame would end 16 bytes past src
             (0, out_bytes),                        # output offset past out_bytes (memory the buffer does hold: it must stay untouched)
             (fb, out_bytes - slot + 16),           # the slot would end 16 bytes past out
             (-16, 4 * step), (0, -16),             # negative offsets
             (fb, 5 * step)]
    status = _convert(src, items, layout, H, W, "bt601", False, out, out_bytes)
    assert status == [0, 1, 0, 1, 1, 1, 1, 1, 0]
    host = buf.cpu().numpy()
    mask = np.ones(host.size, bool)
    for k, f in ((0, 0), (2, 1), (5, 1)):
        lo = guard + k * step
        assert np.array_equal(host[lo:lo + slot].reshape(H, W, 3), _host_bgr(frames[f], layout, H, W, "bt601", False)), k
        mask[lo:lo + slot] = False
    assert (host[mask] == FILL).all()


def test_engine_entry_fills_strided_out_and_refuses_bad_input():
    eng = engine()
    W, H = 48, 20
    rng = np.random.default_rng(29)
    for pixfmt in ("yuv420p", "yuvj422p", "nv12"):
        layout, full = sampling.yuv_layout(pixfmt)
        fb = sampling.yuv_frame_bytes(layout, H, W)
        frames = rng.integers(0, 256, (4, fb), dtype=np.uint8)
        want = np.stack([_host_bgr(f, layout, H, W, "bt709", full) for f in frames])
        got = eng.yuv_to_bgr(torch.from_numpy(frames).cuda(), H, W, pixfmt, matrix="bt709")
        assert np.array_equal(got.cpu().numpy(), want)
        clip = torch.zeros((2, 2, H, W, 3), dtype=torch.uint8, device="cuda")
        assert eng.yuv_to_bgr(frames, H, W, pixfmt, matrix="bt709", out=clip.view(-1, H, W, 3)).data_ptr() == clip.data_ptr()
        assert np.array_equal(clip.view(-1, H, W, 3).cpu().numpy(), want)
    with pytest.raises(ValueError, match="yuv420p10le"):
        eng.yuv_to_bgr(torch.zeros(10, dtype=torch.uint8, device="cuda"), 2, 2, "yuv420p10le")
    with pytest.raises(ValueError, match="whole number"):
        eng.yuv_to_bgr(torch.zeros(7, dtype=torch.uint8, device="cuda"), 2, 2, "yuv420p")
    with pytest.raises(ValueError, match="bt2020"):
        eng.yuv_to_bgr(torch.zeros(6, dtype=torch.uint8, device="cuda"), 2, 2, "yuv420p", matrix="bt2020")


def _video(tmp_path, name, W, H, n, seed, pixfmt="yuv420p"):
    fb = sampling.yuv_frame_bytes(sampling.yuv_layout(pixfmt)[0], H, W)
    p = str(tmp_path / name)
    np.random.default_rng(seed).integers(0, 256, (n, fb), dtype=np.uint8).tofile(p)
    return p


def test_gpu_yuv_loader_equals_load_clip_from_yuv(tmp_path):
    p = _video(tmp_path, "a.yuv", 48, 32, 60, 31)
    for framerate in (25, 2.5):                                    # interval 12: pairs (n, n+1); interval 1: every frame, with itself
        want = sampling.load_clip_from_yuv(p, 48, 32, "yuv420p", framerate)
        loader = sampling.GpuYuvLoader([p], [48], [32], ["yuv420p"], [framerate], device="cuda:0")
        got = loader(0)
        assert len(loader) == 1 and got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == want.shape
        assert np.array_equal(got.cpu().numpy(), want)
        assert torch.equal(loader(0), got)
    dev = video_frames_extract.process_video_residual("live_qualcomm", "a", 12, p, str(tmp_path), 48, 32, "yuv420p", 25, device="cuda:0")
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), sampling.load_clip_from_yuv(p, 48, 32, "yuv420p", 25))
    odd = _video(tmp_path, "odd.yuv", 33, 17, 30, 37, "yuvj422p")     # odd size, full range: the bytewise path
    got = sampling.GpuYuvLoader([odd], 33, 17, "yuvj422p", 30)(0)
    assert np.array_equal(got.cpu().numpy(), sampling.load_clip_from_yuv(odd, 33, 17, "yuvj422p", 30))
    one = _video(tmp_path, "one.yuv", 48, 32, 1, 41)
    with pytest.raises(FileNotFoundError):
        sampling.GpuYuvLoader([one], [48], [32], ["yuv420p"], [25], device="cuda:0")(0)
    with pytest.raises(ValueError, match="uyvy422"):
        sampling.GpuYuvLoader([p], [48], [32], ["uyvy422"], [25], device="cuda:0")(0)


def test_dataset_pass_from_yuv_files_equals_the_resident_clips(tmp_path):
    rn50_weights(), vit_weights("vit_base")
    eng = engine()
    W, H = 320, 240
    paths = [_video(tmp_path, f"v{i}.yuv", W, H, 26 + 12 * i, 50 + i) for i in range(2)]      # T = 3 and 4 at framerate 25
    loader = sampling.GpuYuvLoader(paths, [W] * 2, [H] * 2, ["yuv420p"] * 2, [25, 25], device=eng.device)
    resident = [torch.from_numpy(sampling.load_clip_from_yuv(p, W, H, "yuv420p", 25)).cuda() for p in paths]
    assert [c.shape[0] for c in resident] == [3, 4]
    want, e1 = dataset.extract_dataset_clips(resident, 2, eng, clips_per_step=2, rank=0, world=1)
    got, e2 = dataset.extract_dataset_clips(loader, 2, eng, clips_per_step=2, rank=0, world=1, workers=2)
    assert not e1 and not e2
    assert torch.isfinite(got).all() and torch.equal(got, want)


def test_two_loader_threads_on_their_own_streams_equal_serial_calls(tmp_path):
    paths = [_video(tmp_path, f"t{i}.yuv", 64, 48, 40, 60 + i) for i in range(2)]
    loader = sampling.GpuYuvLoader(paths, 64, 48, "yuv420p", 25, device="cuda:0")
    serial = [loader(i).cpu().numpy() for i in range(2)]
    for i in range(2):
        assert np.array_equal(serial[i], sampling.load_clip_from_yuv(paths[i], 64, 48, "yuv420p", 25))
    errors, streams = [], set()

    def work(k):
        try:
            for r in range(4):
                i = (k + r) % 2
                got = loader(i)
                if not np.array_equal(got.cpu().numpy(), serial[i]):
                    errors.append((k, r, i))
            streams.add(loader._state().stream.cuda_stream)
        except Exception as e:          # noqa: BLE001
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors and len(streams) == 2
