"""The RELAX_YUVF_* formats on the GPU (csrc/yuv.hip: relax_yuv_to_bgr_ex; csrc/greyscale.hip: relax_yuv_greyscale_scan_ex;
RelaxEngine.yuv_to_bgr_ex / yuv_greyscale_scan_ex; sampling.GpuYuvLoader and check_greyscale.scan_yuv_file with extended=True)
against the numpy statement (sampling.yuv_samples + sampling.yuv_frame_bgr_ex): bit for bit, through the C-ABI."""
import ctypes as C

import numpy as np
import pytest
import torch

from relax_vqa_amd import _lib, sampling
from relax_vqa_amd.data_processing import check_greyscale
from tests import yuv_ex_cases as cases
from tests.gpu_common import engine

pytestmark = pytest.mark.gpu

FILL = 0xA5
PRESET = 0x7f


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _aligned(nbytes):
    """A device byte buffer whose first byte lies at a 16-byte-aligned address."""
    raw = torch.zeros(nbytes + 32, dtype=torch.uint8, device="cuda")
    shift = (-raw.data_ptr()) % 16
    return raw[shift:shift + nbytes]


def _upload(host):
    dev = _aligned(host.size)
    dev.copy_(torch.from_numpy(host))
    return dev


def _convert(entry, src, items, fmt, H, W, matrix, full_range, out, out_bytes):
    """relax_yuv_to_bgr_ex (or relax_yuv_to_bgr) on device tensors; -> status words (host)."""
    lib = _lib.load()
    dev_items = torch.tensor(items, dtype=torch.int64).reshape(-1, 2).cuda()
    status = torch.full((len(items),), -7, dtype=torch.int32, device="cuda")
    rc = getattr(lib, entry)(C.c_void_p(src.data_ptr()), src.numel(), C.c_void_p(dev_items.data_ptr()), len(items), fmt, H, W,
                             sampling.YUV_MATRICES[matrix], int(full_range), C.c_void_p(out.data_ptr()), out_bytes,
                             C.c_void_p(status.data_ptr()), _stream())
    assert rc == 0, lib.relax_last_error(None).decode()
    return status.cpu().tolist()


def _scan(entry, src, offsets, fmt, H, W, matrix, full_range):
    lib = _lib.load()
    off = torch.tensor(offsets, dtype=torch.int64).cuda()
    out = torch.full((len(offsets) * 8 * 4,), PRESET, dtype=torch.uint8, device="cuda")
    rc = getattr(lib, entry)(C.c_void_p(src.data_ptr()), src.numel(), C.c_void_p(off.data_ptr()), len(offsets), fmt, H, W,
                             sampling.YUV_MATRICES[matrix], int(full_range), C.c_void_p(out.data_ptr()), _stream())
    assert rc == 0, lib.relax_last_error(None).decode()
    return out.view(torch.int32).reshape(-1, 8)


def _bgr_scan(bgr, N, H, W):
    lib = _lib.load()
    out = torch.full((N * 8 * 4,), PRESET, dtype=torch.uint8, device="cuda")
    rc = lib.relax_greyscale_scan(C.c_void_p(bgr.data_ptr()), H * W * 3, N, H, W, C.c_void_p(out.data_ptr()), _stream())
    assert rc == 0, lib.relax_last_error(None).decode()
    return out.view(torch.int32).reshape(-1, 8)


@pytest.mark.parametrize("name", cases.NEW_NAMES)
def test_bit_equal_to_numpy_in_strided_slots(name):
    """Three frames back to back in an aligned buffer (the 16-byte path wherever W is a multiple of 16 and frame_bytes one too) and
    a copy of frame 0 one byte past them - for 2-byte samples a second copy two bytes off - so the bytewise path runs at every
    size; written into the strided slots of a tensor between guard bytes: every slot equals numpy, no other byte changes."""
    fmt, _ = cases.fmt(name)
    for W, H in cases.GPU_SIZES:
        fb = cases.frame_bytes(name, H, W)
        frames = cases.random_frames(name, H, W, 3, 17 + W)
        pad = (-(3 * fb + 1 + fb)) % 16 + 2                                   # the second copy: two bytes past a 16-byte boundary
        src = np.concatenate([frames.reshape(-1), np.zeros(1, np.uint8), frames[0], np.zeros(pad, np.uint8), frames[0]])
        offsets = [0, fb, 2 * fb, 3 * fb + 1] + ([4 * fb + 1 + pad] if name in cases.TWO_BYTE else [])
        assert name not in cases.TWO_BYTE or offsets[4] % 16 == 2
        n_items = len(offsets)
        slot, guard, tail = H * W * 3, 64, 256
        buf = torch.full((guard + n_items * (slot + guard) + tail,), FILL, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        out = buf[guard:]
        order = [2, 0, 3, 1, 4][:n_items]                                     # item n goes to slot order[n]
        items = [(offsets[n], order[n] * (slot + guard)) for n in range(n_items)]
        out_bytes = (n_items - 1) * (slot + guard) + slot                     # ends with the last slot: its guard and the tail lie past `out`
        dev = _upload(src)
        for matrix, full in (cases.COMBOS if H * W <= cases.SMALL else cases.COMBOS[:1]):
            buf.fill_(FILL)
            status = _convert("relax_yuv_to_bgr_ex", dev, items, fmt, H, W, matrix, full, out, out_bytes)
            assert status == [0] * n_items, (W, H)
            host = buf.cpu().numpy()
            mask = np.ones(host.size, bool)
            wants = [cases.host_bgr(f, name, H, W, matrix, full) for f in frames]
            for n in range(n_items):
                lo = guard + order[n] * (slot + guard)
                assert np.array_equal(host[lo:lo + slot].reshape(H, W, 3), wants[n] if n < 3 else wants[0]), (W, H, n, matrix, full)
                mask[lo:lo + slot] = False
            assert (host[mask] == FILL).all(), (W, H)


@pytest.mark.parametrize("full_range", [False, True], ids=["limited", "full"])
def test_every_luma_in_one_4096_frame_and_the_extremes(full_range):
    """One 4096 x 4096 yuv444p10le frame: every Y with 128 values each of U and V (every 8th and the top); and a 64 x 64 frame of the
    extremes 0 / 1023 of each."""
    eng = engine()
    c = np.minimum(np.arange(128) * 8 + (np.arange(128) == 127) * 7, 1023).astype(np.uint16)
    y, u, v = np.meshgrid(np.arange(1024, dtype=np.uint16), c, c, indexing="ij")
    frame = np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]).view(np.uint8)
    if full_range:                                                            # no 10-bit yuvj name: the range through the C entry
        got = torch.empty((1, 4096, 4096, 3), dtype=torch.uint8, device="cuda")
        assert _convert("relax_yuv_to_bgr_ex", torch.from_numpy(frame).cuda(), [(0, 0)], 11, 4096, 4096, "bt601", True, got, got.numel()) == [0]
    else:
        got = eng.yuv_to_bgr_ex(torch.from_numpy(frame).cuda(), 4096, 4096, "yuv444p10le")
    want = sampling.yuv_frame_bgr_ex(y.reshape(4096, 4096), u.reshape(4096, 4096), v.reshape(4096, 4096), 10, full_range=full_range)
    assert tuple(got.shape) == (1, 4096, 4096, 3) and torch.equal(got[0].cpu(), torch.from_numpy(want))
    e = np.array([0, 1023], np.uint16)
    y, u, v = (a.reshape(-1) for a in np.meshgrid(e, e, e, indexing="ij"))
    y, u, v = (np.tile(a, 512).reshape(64, 64) for a in (y, u, v))
    frame = np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]).view(np.uint8)
    for matrix in ("bt601", "bt709"):
        out = torch.empty((64, 64, 3), dtype=torch.uint8, device="cuda")
        assert _convert("relax_yuv_to_bgr_ex", _upload(frame), [(0, 0)], 11, 64, 64, matrix, full_range, out, out.numel()) == [0]
        assert np.array_equal(out.cpu().numpy(), sampling.yuv_frame_bgr_ex(y, u, v, 10, matrix=matrix, full_range=full_range))


@pytest.mark.parametrize("layout", [0, 1, 2, 3])
def test_formats_0_to_3_through_ex_equal_the_old_entries(layout):
    for W, H in ((34, 18), (64, 32)):
        fb = sampling.yuv_frame_bytes(layout, H, W)
        assert sampling.yuv_frame_bytes_ex(layout, H, W) == fb
        frames = np.random.default_rng(5 + W).integers(0, 256, (3, fb), dtype=np.uint8)
        dev = _upload(frames.reshape(-1))
        slot = H * W * 3
        items = [(n * fb, n * slot) for n in range(3)]
        for matrix, full in cases.COMBOS:
            a, b = (torch.full((3 * slot,), FILL, dtype=torch.uint8, device="cuda") for _ in range(2))
            assert _convert("relax_yuv_to_bgr", dev, items, layout, H, W, matrix, full, a, a.numel()) == [0, 0, 0]
            assert _convert("relax_yuv_to_bgr_ex", dev, items, layout, H, W, matrix, full, b, b.numel()) == [0, 0, 0]
            assert torch.equal(a, b)
            offs = [n * fb for n in range(3)]
            assert torch.equal(_scan("relax_yuv_greyscale_scan", dev, offs, layout, H, W, matrix, full),
                               _scan("relax_yuv_greyscale_scan_ex", dev, offs, layout, H, W, matrix, full))


@pytest.mark.parametrize("name", ["yuv420p10le", "uyvy422"])
def test_out_of_range_items_write_nothing_and_spare_the_call(name):
    W, H = 64, 32
    fmt, _ = cases.fmt(name)
    fb, slot, guard = cases.frame_bytes(name, H, W), H * W * 3, 64
    frames = cases.random_frames(name, H, W, 2, 23)
    src = _upload(frames.reshape(-1))
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
    status = _convert("relax_yuv_to_bgr_ex", src, items, fmt, H, W, "bt601", False, out, out_bytes)
    assert status == [0, 1, 0, 1, 1, 1, 1, 1, 0]
    host = buf.cpu().numpy()
    mask = np.ones(host.size, bool)
    for k, f in ((0, 0), (2, 1), (5, 1)):
        lo = guard + k * step
        assert np.array_equal(host[lo:lo + slot].reshape(H, W, 3), cases.host_bgr(frames[f], name, H, W)), k
        mask[lo:lo + slot] = False
    assert (host[mask] == FILL).all()
    offsets = [0, 2 * fb, fb, fb + 16, -16, fb]
    got = _scan("relax_yuv_greyscale_scan_ex", src, offsets, fmt, H, W, "bt601", False).cpu().numpy()
    assert got[:, 6].tolist() == [0, 1, 0, 1, 1, 0] and not got[[1, 3, 4], :6].any() and not got[:, 7].any()
    assert np.array_equal(got[[0, 2, 5]], cases.records(np.stack([cases.host_bgr(frames[f], name, H, W) for f in (0, 1, 1)])))


SCAN_SIZES = [(2, 16), (6, 48), (7, 50), (3, 17)]        # H, W: the lane, a partial group of 4:1:0's four rows, the bytewise path


@pytest.mark.parametrize("name", cases.NEW_NAMES)
def test_fused_scan_equals_the_scan_of_the_converted_frames(name):
    """Colour frames, grey frames, and the two frames on either side of the threshold; at aligned slots and one byte off."""
    fmt, _ = cases.fmt(name)
    for H, W in SCAN_SIZES:
        fb = cases.frame_bytes(name, H, W)
        grey_a, colour_a = cases.threshold_frames(name, H, W, 3 + H)
        frames = np.stack(list(cases.random_frames(name, H, W, 2, 7 + H)) + [cases.grey_frame(name, H, W, 11 + H), grey_a, colour_a])
        N = len(frames)
        slot = (fb + 15) // 16 * 16
        packed = np.concatenate([np.zeros(1, np.uint8), frames.reshape(-1)])          # frame n at 1 + n * fb: unaligned
        padded = np.zeros(N * slot, np.uint8)                                         # frame n at n * slot: aligned
        for n in range(N):
            padded[n * slot:n * slot + fb] = frames[n]
        for offsets, host in (([1 + n * fb for n in range(N)], packed), ([n * slot for n in range(N)], padded)):
            src = _upload(host)
            for matrix, full in cases.COMBOS:
                fused = _scan("relax_yuv_greyscale_scan_ex", src, offsets, fmt, H, W, matrix, full)
                bgr = _aligned(N * H * W * 3)
                items = [(o, n * H * W * 3) for n, o in enumerate(offsets)]
                assert _convert("relax_yuv_to_bgr_ex", src, items, fmt, H, W, matrix, full, bgr, bgr.numel()) == [0] * N
                assert torch.equal(fused, _bgr_scan(bgr, N, H, W)), (name, H, W, matrix, full, offsets[0])
                want = cases.records(np.stack([cases.host_bgr(f, name, H, W, matrix, full) for f in frames]))
                assert np.array_equal(fused.cpu().numpy(), want), (name, H, W, matrix, full, offsets[0])
                if (matrix, full) == ("bt601", False):
                    assert not want[2, :6].any() and want[3, 3:6].max() <= 3 < want[4, 3:6].max()


def _video(tmp_path, name, W, H, n, seed):
    p = str(tmp_path / f"{name}_{W}x{H}.yuv")
    cases.random_frames(name, H, W, n, seed).tofile(p)
    return p


@pytest.mark.parametrize("name,W,H,framerate", [("yuv420p10le", 48, 32, 25), ("uyvy422", 33, 17, 30), ("yuv410p", 34, 18, 2.5)])
def test_gpu_yuv_loader_extended_equals_load_clip_from_yuv(tmp_path, name, W, H, framerate):
    p = _video(tmp_path, name, W, H, 40, 31)
    want = sampling.load_clip_from_yuv(p, W, H, name, framerate, extended=True)
    loader = sampling.GpuYuvLoader([p], [W], [H], [name], [framerate], device="cuda:0", extended=True)
    got = loader(0)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(loader(0), got)                                        # a second call: the same bits
    eng = engine()
    frames = np.fromfile(p, np.uint8)
    all_bgr = eng.yuv_to_bgr_ex(frames, H, W, name)
    assert np.array_equal(all_bgr.cpu().numpy(), sampling.load_frames_from_yuv(p, W, H, name, list(range(40)), extended=True))
    assert torch.equal(eng.yuv_greyscale_scan_ex(frames, H, W, name)["records"], eng.greyscale_scan(all_bgr)["records"])
    with pytest.raises(ValueError, match="whole number"):
        eng.yuv_to_bgr_ex(torch.zeros(7, dtype=torch.uint8, device="cuda"), H, W, name)
    with pytest.raises(ValueError, match="out must"):
        eng.yuv_to_bgr_ex(frames, H, W, name, out=torch.empty((40, H, W, 3), dtype=torch.uint8, device="cuda")[:, :, :, :2])


def test_default_surface_still_refuses(tmp_path):
    p = _video(tmp_path, "uyvy422", 48, 32, 30, 3)
    with pytest.raises(ValueError, match="uyvy422"):
        sampling.GpuYuvLoader([p], [48], [32], ["uyvy422"], [25], device="cuda:0")(0)
    with pytest.raises(ValueError, match="yuv420p10le"):
        engine().yuv_to_bgr(torch.zeros(12, dtype=torch.uint8, device="cuda"), 2, 2, "yuv420p10le")
    with pytest.raises(ValueError, match="yuv420p10le"):
        check_greyscale.scan_yuv_file(p, 48, 32, "yuv420p10le")
    lib = _lib.load()
    one = torch.zeros(64, dtype=torch.uint8, device="cuda")
    items = torch.zeros(2, dtype=torch.int64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    for entry, bad in (("relax_yuv_to_bgr", 9), ("relax_yuv_to_bgr_ex", 16), ("relax_yuv_to_bgr_ex", -1)):
        rc = getattr(lib, entry)(C.c_void_p(one.data_ptr()), 64, C.c_void_p(items.data_ptr()), 1, bad, 2, 2, 0, 0, C.c_void_p(one.data_ptr()), 12,
                                 C.c_void_p(status.data_ptr()), _stream())
        assert rc != 0 and str(bad) in lib.relax_last_error(None).decode()


@pytest.mark.parametrize("colour_at", [None, 17])
def test_scan_yuv_file_extended_on_a_10_bit_file(tmp_path, colour_at):
    name, W, H, n = "yuv420p10le", 48, 8, 24
    frames = np.stack([cases.grey_frame(name, H, W, 100 + k) for k in range(n)])
    if colour_at is not None:
        frames[colour_at] = cases.random_frames(name, H, W, 1, 9)[0]
    path = str(tmp_path / f"grey{colour_at}.yuv")
    frames.tofile(path)
    host = cases.records(sampling.load_frames_from_yuv(path, W, H, name, list(range(n)), extended=True))
    res = check_greyscale.scan_yuv_file(path, W, H, name, chunk_frames=7, stop_at_colour=False, extended=True)
    assert res["n_frames"] == n and res["frames_scanned"] == n and np.array_equal(res["records"], host)
    assert res["first_colour_frame"] == colour_at
    assert check_greyscale.check_video_greyscale(path, W, H, name, chunk_frames=7, extended=True) == (colour_at is None, True)
