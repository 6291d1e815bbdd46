"""relax_png_encode on the device against the host build of the same core (tests/png_encode_driver.py, whose bytes
tests/test_png_encode_cpu.py checks against zlib, Pillow and numpy): the device must give the same bytes, lengths and
statuses; then the host layer over it (pngencode.py, RelaxEngine.encode_png / write_png) and the round trip through the
GPU decoder."""
import ctypes as C
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import png_encode_driver as drv
from tests.gpu_common import engine, vit_weights

pytestmark = pytest.mark.gpu


def encode_device(imgs, filters=None, capacities=None, scratch_fill=0xFF):
    """tests/png_encode_driver.encode_host, on the device through the C-ABI: the same layout, the same sentinel bytes."""
    eng = engine()
    filters = [-1] * len(imgs) if filters is None else list(filters)
    flat, items, out_bytes, scratch_bytes = drv.layout(imgs, filters, capacities)
    dev = eng.device
    d_flat, d_items = torch.from_numpy(flat).to(dev), torch.from_numpy(items).to(dev)
    out = torch.full((out_bytes,), 0xEE, dtype=torch.uint8, device=dev)
    scratch = torch.full((scratch_bytes,), scratch_fill, dtype=torch.uint8, device=dev)
    lengths = torch.full((len(imgs),), -1, dtype=torch.int64, device=dev)
    status = torch.full((len(imgs),), -1, dtype=torch.int32, device=dev)
    rc = eng.lib.relax_png_encode(C.c_void_p(d_flat.data_ptr()), flat.size, C.c_void_p(d_items.data_ptr()), len(imgs),
                                  C.c_void_p(out.data_ptr()), out_bytes, C.c_void_p(scratch.data_ptr()), scratch_bytes,
                                  C.c_void_p(lengths.data_ptr()), C.c_void_p(status.data_ptr()),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, eng.lib.relax_last_error(None).decode()
    torch.cuda.synchronize()
    out, lengths, status = out.cpu().numpy(), lengths.cpu().numpy(), status.cpu().numpy()
    streams = [bytes(out[items[n, 5]:items[n, 5] + lengths[n]]) if status[n] == 0 else None for n in range(len(imgs))]
    return streams, lengths, status, out, items


@pytest.fixture(scope="module")
def device_results():
    cs = drv.cases()
    return encode_device([c[1] for c in cs], [c[2] for c in cs])


def test_bound_is_the_host_builds():
    eng = engine()
    for H, W, Cc, f in ((1, 1, 1, -1), (224, 224, 3, 2), (2160, 3840, 3, -1), (2, 5461, 3, 0), (4, 5462, 3, -1), (4, 4, 4, -1)):
        assert drv.bound(H, W, Cc, f, eng.lib.relax_png_encode_bound) == drv.bound(H, W, Cc, f)


def test_device_bytes_are_the_host_builds(device_results):
    streams, lengths, status, _, _ = device_results
    want, want_len, want_status = drv.host_results()
    assert status.tolist() == want_status.tolist() and lengths.tolist() == want_len.tolist()
    for (name, _, _), got, ref in zip(drv.cases(), streams, want):
        assert got == ref, name


def test_a_second_call_gives_the_same_bytes(device_results):
    cs = drv.cases()
    assert encode_device([c[1] for c in cs], [c[2] for c in cs])[0] == device_results[0]


def test_scratch_contents_do_not_matter(device_results):
    """The fixture's call starts from a scratch of 0xFF bytes; one of 0x00 and one of 0xA5 bytes give the same streams."""
    cs = drv.cases()
    for fill in (0x00, 0xA5):
        assert encode_device([c[1] for c in cs], [c[2] for c in cs], scratch_fill=fill)[0] == device_results[0]


def test_mixed_call_with_bad_items():
    imgs = [drv.content("mixed", 12, 224, 3, 1), drv.content("noise", 9, 17, 1, 2), drv.content("mixed", 224, 224, 1, 3),
            np.zeros((4, 4, 4), np.uint8), drv.content("hgrad", 5, 3, 1, 4), drv.golden_crop(90, 224, 3, 5)]
    filters = [-1, 3, 4, -1, 0, -1]
    full = len(drv.encode_host([imgs[1]], [3])[0][0])
    caps = [None, full - 1, None, 64, None, None]
    got, got_len, got_status, out, items = encode_device(imgs, filters, caps)
    want, want_len, want_status, want_out, _ = drv.encode_host(imgs, filters, caps)
    assert got_status.tolist() == want_status.tolist() == [0, drv.OUT_TOO_SMALL, 0, drv.BAD_ARGS, 0, 0]
    assert got_len.tolist() == want_len.tolist() and got == want
    assert np.array_equal(out, want_out)            # the sentinel bytes around and between the streams included


def test_strided_clip_slots_and_round_trip_through_the_decoder():
    eng = engine()
    clip = torch.from_numpy(np.stack([np.stack([drv.golden_crop(60, 100, 3, k), drv.content("mixed", 60, 100, 3, k)])
                                      for k in range(3)])).to(eng.device)             # [T,2,H,W,3]
    firsts = clip[:, 0]                                                                # strided slots, packed rows
    stats = {}
    files = eng.encode_png(firsts, stats=stats)
    assert stats == {"gpu": 3, "fallback": 0}
    want = drv.encode_host([f.cpu().numpy() for f in firsts])[0]
    for data, z, img in zip(files, want, firsts):
        from relax_vqa_amd import png
        assert png.parse(data).zdata == z
        with Image.open(io.BytesIO(data)) as im:
            assert np.array_equal(np.asarray(im)[..., ::-1], img.cpu().numpy())
    back = eng.decode_png(files)
    assert torch.equal(back, firsts)
    gray = clip[:, 1, :, :, 1]                                                         # [T,H,W] with a pixel stride of 3: repacked
    back = eng.decode_png(eng.encode_png(gray))
    assert torch.equal(back, gray.unsqueeze(-1).expand(-1, -1, -1, 3))                 # gray comes back replicated
    sizes = [clip[0, 0], clip[1, 1, :7, :9], clip[2, 0, :, :, 0]]                      # a list of differing sizes and channels
    for data, img in zip(eng.encode_png(sizes, filter=4), sizes):
        with Image.open(io.BytesIO(data)) as im:
            a = np.asarray(im)
        assert np.array_equal(a if a.ndim == 2 else a[..., ::-1], img.cpu().numpy())


def test_refused_geometry_is_written_by_pillow_and_counted(tmp_path):
    eng = engine()
    wide = torch.from_numpy(drv.content("hgrad", 2, 5462, 3, 1)).to(eng.device)        # rows of 16386 bytes
    ok = torch.from_numpy(drv.content("hgrad", 2, 5461, 3, 1)).to(eng.device)
    stats = {}
    paths = [str(tmp_path / "wide.png"), str(tmp_path / "ok.png")]
    eng.write_png(paths, [wide, ok], stats=stats)
    assert stats == {"gpu": 1, "fallback": 1}
    for p, img in zip(paths, (wide, ok)):
        with Image.open(p) as im:
            assert np.array_equal(np.asarray(im)[..., ::-1], img.cpu().numpy())


def test_attention_overlay_frame_at_1080p_written_and_read_back(tmp_path):
    eng = engine()
    vit_weights("vit_base")
    frame = np.tile(drv.golden_frames()[1], (1, 1, 1))[:1080, :1920]
    assert frame.shape == (1080, 1920, 3)
    frames = torch.from_numpy(np.stack([frame, np.roll(frame, 3, axis=1)])[None]).to(eng.device)
    overlay = eng.attention_overlays(frames, "ori_frag")["overlay"]
    path = str(tmp_path / "overlay.png")
    eng.write_png([path], overlay)
    with Image.open(path) as im:
        assert np.array_equal(np.asarray(im)[..., ::-1], overlay[0].cpu().numpy())
    assert os.path.getsize(path) < overlay[0].numel()
    assert torch.equal(eng.decode_png([path]), overlay)


def _golden(stem, suffix):
    with Image.open(os.path.join(drv.GOLDEN, "png_" + stem, f"{stem}{suffix}.png")) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[..., ::-1])


@pytest.mark.parametrize("stem", ["5636101558_3", "TelevisionClip_1080P-68c6_1"])
def test_write_example_set_on_the_golden_pairs(tmp_path, stem):
    from relax_vqa_amd import visualisation
    eng = engine()
    video, number = stem.rsplit("_", 1)
    frames = torch.from_numpy(np.stack([_golden(stem, ""), _golden(stem, "_next")])[None]).to(eng.device)
    paths = visualisation.write_example_set(eng, frames, str(tmp_path), video, numbers=[int(number)])
    arrays = visualisation.example_set_arrays(eng, frames)
    assert set(paths) == set(visualisation.NAMES)
    # the file names are the golden set's (which has no _residual.png for the 1080p pair; the reference writes one)
    golden_names = {n for n in os.listdir(os.path.join(drv.GOLDEN, "png_" + stem)) if n not in (stem + ".png", stem + "_next.png")}
    assert golden_names <= set(os.listdir(tmp_path)) == {os.path.basename(p[0]) for p in paths.values()}
    for suffix, (path,) in paths.items():
        with Image.open(path) as im:
            got = np.asarray(im)[..., ::-1]
        assert np.array_equal(got, arrays[suffix][0].cpu().numpy()), suffix        # the engine's own array, bit for bit
        # the kinds tests/test_gpu_reference_png_sets.py holds bit-equal to the reference's files
        if suffix in ("residual_imp", "ori_frag") or (suffix == "residual" and f"{stem}_residual.png" in golden_names):
            assert np.array_equal(got, _golden(stem, "_" + suffix)), suffix


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("driver", ["main_fragment_layerstack", "main_fragment_pool", "main_residual", "demo_test"])
def test_driver_flag_off_writes_nothing_and_on_writes_the_files(tmp_path, driver):
    import importlib

    from relax_vqa_amd import runtime, synth, visualisation
    mod = importlib.import_module("relax_vqa_amd." + driver)
    clip = synth.synthetic_clip(1, 272, 400, clip_id=7)
    flag = (str(tmp_path / "on"), "video", [5])
    names = visualisation.NAMES
    if driver == "demo_test":
        # the demo driver's switch sits on the engine it runs on (RelaxEngine.demo_write_png, read by full_clip_vector)
        z = np.load(os.path.join(drv.GOLDEN, "mlp_head.npz"))
        runtime.set_weights(resnet50=synth.resnet50_state_dict(), vit=synth.vit_state_dict("vit_base"), vit_name="vit_base")
        mod.load_head(synth.mlp_head_state_dict(35203, 256, seed=23), z["imputer_statistics"], (z["scale"], z["min"]))
        names = visualisation.NAMES[:3]             # flow=False below: no flow kinds

        def call(write_png=None):
            runtime.get_engine().demo_write_png = write_png
            try:
                return mod.evaluate_video_quality(clip, "konvid_1k", flow=False)
            finally:
                runtime.get_engine().demo_write_png = None
    elif driver == "main_residual":
        runtime.set_weights(resnet50=synth.resnet50_state_dict())

        def call(write_png=None):               # a module flag here: process_pair keeps the reference's parameter list
            mod.WRITE_PNG = write_png
            try:
                return mod.process_pair(clip[0, 0], clip[0, 1], "resnet50", "frame_diff")
            finally:
                mod.WRITE_PNG = None
    else:
        def call(**kw):
            return mod.fragment_pair(clip[0, 0], clip[0, 1], **kw)
    before = set(os.listdir(tmp_path))
    off = call()
    assert set(os.listdir(tmp_path)) == before
    on = call(write_png=flag)
    assert _same(off, on)
    assert sorted(os.listdir(flag[0])) == sorted(f"video_5_{s}.png" for s in names)
    with Image.open(os.path.join(flag[0], "video_5_residual.png")) as im:
        want = np.abs(clip[0, 1].astype(np.int16) - clip[0, 0].astype(np.int16)).astype(np.uint8)
        assert np.array_equal(np.asarray(im)[..., ::-1], want)
