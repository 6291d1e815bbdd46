"""The GPU PNG decoder (csrc/png_decode.hip: relax_png_decode, RelaxEngine.decode_png, sampling.GpuFrameLoader) against
sampling.read_frame_bgr - cv2.imread's bytes - on the test corpus of tests/png_corpus.py and the committed golden frames; strided
writes into clip slots, the malformed streams' status codes, the host fallback, the clip loader and a dataset pass.
Every malformed stream here was first shown to be rejected cleanly by the sanitized host build (test_png_decode_sanitized.py)."""
import glob
import io
import os
import shutil
import threading

import numpy as np
import pytest
import torch
from PIL import Image

from relax_vqa_amd import dataset, png, pngdecode, sampling
from tests import png_corpus
from tests.gpu_common import engine, rn50_weights, synth, vit_weights

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def test_corpus_in_one_mixed_batch_is_bit_exact(tmp_path):
    corpus = png_corpus.corpus()
    paths = [_write(tmp_path, f"{name}.png", data) for name, data, _ in corpus]
    stats = {}
    got = engine().decode_png(paths, stats=stats)
    assert isinstance(got, list) and len(got) == len(corpus) and stats == {"gpu": len(corpus), "fallback": 0}
    for p, g, (name, _, want) in zip(paths, got, corpus):
        ref = sampling.read_frame_bgr(p)
        assert np.array_equal(ref, want), name
        assert g.is_cuda and g.dtype == torch.uint8 and np.array_equal(g.cpu().numpy(), ref), name


def test_golden_frames_are_bit_exact():
    paths = sorted(glob.glob(os.path.join(GOLDEN, "png_*", "*.png")))
    assert len(paths) >= 20
    got = engine().decode_png(paths)
    for p, g in zip(paths, got):
        assert np.array_equal(g.cpu().numpy(), sampling.read_frame_bgr(p)), p


def test_same_size_batch_and_bytes_sources():
    a = os.path.join(GOLDEN, "png_5636101558_3", "5636101558_3.png")
    b = os.path.join(GOLDEN, "png_5636101558_3", "5636101558_3_next.png")
    got = engine().decode_png([a, open(b, "rb").read(), a])
    assert tuple(got.shape) == (3, 540, 960, 3)
    assert np.array_equal(got[0].cpu().numpy(), sampling.read_frame_bgr(a))
    assert np.array_equal(got[1].cpu().numpy(), sampling.read_frame_bgr(b))
    assert torch.equal(got[0], got[2])


def test_strided_slots_leave_guard_bytes_alone():
    """Frames decoded straight into the slots of a clip tensor [T,2,H,W,3] that sits inside a larger buffer with guard bytes
    between the slots: every slot equals read_frame_bgr, no other byte changes."""
    frames = [os.path.join(GOLDEN, "png_TelevisionClip_1080P-68c6_1", f) for f in
              ("TelevisionClip_1080P-68c6_1.png", "TelevisionClip_1080P-68c6_1_next.png", "TelevisionClip_1080P-68c6_1_residual_of.png")]
    H, W = 1080, 1920
    slot, guard = H * W * 3, 4096
    T = 3
    buf = torch.full((guard + T * 2 * (slot + guard),), 0xA5, dtype=torch.uint8, device="cuda")
    view = buf[guard:].as_strided((T, 2, H, W, 3), (2 * (slot + guard), slot + guard, W * 3, 3, 1))
    srcs = [frames[k % 3] for k in range(2 * T)]
    engine().decode_png(srcs, out=torch.as_strided(view, (2 * T, H, W, 3), (slot + guard, W * 3, 3, 1)))
    host = buf.cpu().numpy()
    mask = np.ones(host.size, bool)
    for k in range(2 * T):
        lo = guard + k * (slot + guard)
        assert np.array_equal(host[lo:lo + slot].reshape(H, W, 3), sampling.read_frame_bgr(srcs[k])), k
        mask[lo:lo + slot] = False
    assert (host[mask] == 0xA5).all()


def test_malformed_streams_give_their_status_and_spare_the_batch(tmp_path):
    good = png_corpus.corpus()[::5]
    bad = png_corpus.malformed()
    srcs, want = [], []
    for i, case in enumerate(bad):
        name, data, ref = good[i % len(good)]
        srcs += [data, png_corpus.malformed_png(case)]
        want += [0, case[5]]
    statuses = []
    got = engine().decode_png(srcs, statuses=statuses)
    assert statuses == want, [(c[0], s) for c, s in zip(bad, statuses[1::2])]
    for i in range(len(bad)):
        ref = good[i % len(good)][2]
        assert np.array_equal(got[2 * i].cpu().numpy(), ref), good[i % len(good)][0]
    p = _write(tmp_path, "broken.png", png_corpus.malformed_png(bad[0]))
    with pytest.raises(pngdecode.PngDecodeError, match="broken.png.*truncated zlib stream"):
        engine().decode_png([p])


def _pillow_file(tmp_path, name, im, **kw):
    p = str(tmp_path / name)
    im.save(p, format="PNG", **kw)
    return p


def test_fallback_files_equal_read_frame_bgr_and_are_counted(tmp_path):
    rng = np.random.default_rng(5)
    pal = Image.fromarray(rng.integers(0, 256, (31, 45), dtype=np.uint8), "L").convert("P")
    deep = Image.fromarray(rng.integers(0, 65536, (31, 45), dtype=np.uint16))
    la = Image.fromarray(rng.integers(0, 256, (31, 45, 2), dtype=np.uint8), "LA")
    rgb = Image.fromarray(rng.integers(0, 256, (31, 45, 3), dtype=np.uint8), "RGB")
    paths = [_pillow_file(tmp_path, "p.png", pal), _pillow_file(tmp_path, "rgb.png", rgb), _pillow_file(tmp_path, "d.png", deep),
             _pillow_file(tmp_path, "la.png", la)]
    assert [png.parse(open(p, "rb").read()).channels for p in paths] == [None, 3, None, None]
    stats = {}
    got = engine().decode_png(paths, stats=stats)
    assert stats == {"gpu": 1, "fallback": 3}
    for p, g in zip(paths, got):
        assert np.array_equal(g.cpu().numpy(), sampling.read_frame_bgr(p)), p


def _clip_dir(tmp_path):
    """A sampled-frame directory from the golden 540p pair: frames 0, 12, 24 (and their _next), some mirrored."""
    d = tmp_path / "frames"
    d.mkdir()
    src = os.path.join(GOLDEN, "png_5636101558_3")
    a, b = sampling.read_frame_bgr(os.path.join(src, "5636101558_3.png")), sampling.read_frame_bgr(os.path.join(src, "5636101558_3_next.png"))
    shutil.copy(os.path.join(src, "5636101558_3.png"), d / "vid_0.png")
    shutil.copy(os.path.join(src, "5636101558_3_next.png"), d / "vid_0_next.png")
    Image.fromarray(np.ascontiguousarray(b[:, ::-1, ::-1])).save(d / "vid_12.png", compress_level=3)
    Image.fromarray(np.ascontiguousarray(a[::-1, :, ::-1])).save(d / "vid_12_next.png", compress_level=1)
    Image.fromarray(np.ascontiguousarray(a[..., ::-1])).convert("P").save(d / "vid_24.png")       # a fallback frame
    Image.fromarray(np.ascontiguousarray(b[..., ::-1])).save(d / "vid_24_next.png")
    return str(d)


def test_gpu_frame_loader_equals_load_clip_from_frames(tmp_path):
    d = _clip_dir(tmp_path)
    loader = sampling.GpuFrameLoader(d, ["vid"], device="cuda:0")
    got = loader(0)
    want = sampling.load_clip_from_frames(d, "vid")
    assert got.is_cuda and tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy(), want)
    assert loader.fallbacks == 1
    eng = engine()
    fg, fw = eng.fragment_pairs(got), eng.fragment_pairs(torch.from_numpy(want).cuda())
    for k in fg:
        assert torch.equal(fg[k], fw[k]), k
    Image.new("RGB", (64, 48)).save(os.path.join(d, "vid_36.png"))
    Image.new("RGB", (64, 48)).save(os.path.join(d, "vid_36_next.png"))
    with pytest.raises(ValueError, match="frame sizes differ"):
        loader(0)
    with pytest.raises(FileNotFoundError):
        sampling.GpuFrameLoader(d, ["nothing"], device="cuda:0")(0)


def test_dataset_pass_with_the_gpu_loader_equals_the_pillow_pass(tmp_path):
    rn50_weights(), vit_weights("vit_base")
    eng = engine()
    arrays = [synth.synthetic_clip(t, 240, 320, clip_id=700 + i) for i, t in enumerate((2, 1, 3, 2))]
    for v, c in enumerate(arrays):
        d = tmp_path / f"video{v}"
        d.mkdir()
        for k in range(c.shape[0]):
            Image.fromarray(c[k, 0][..., ::-1]).save(d / f"clip_{k * 12}.png", compress_level=3)
            Image.fromarray(c[k, 1][..., ::-1]).save(d / f"clip_{k * 12}_next.png", compress_level=3)
    # clip 3: one frame's image data corrupted (its CRC recomputed: the container is valid, the zlib stream is not)
    p = tmp_path / "video3" / "clip_12.png"
    info = png.parse(p.read_bytes())
    z = bytearray(info.zdata)
    z[len(z) // 2:len(z) // 2 + 64] = bytes(64)
    p.write_bytes(png_corpus.container(bytes(z), info.width, info.height, info.color_type))
    names = [f"video{v}" for v in range(4)]
    pillow, e1 = dataset.extract_dataset_clips(lambda i: sampling.load_clip_from_frames(str(tmp_path / names[i]), "clip"), 3, eng,
                                               clips_per_step=2, rank=0, world=1)
    loaders = [sampling.GpuFrameLoader(str(tmp_path / n), ["clip"], device=eng.device) for n in names]
    gpu, e2 = dataset.extract_dataset_clips(lambda i: loaders[i](0), 4, eng, clips_per_step=2, rank=0, world=1, workers=3)
    assert not e1 and torch.equal(gpu[:3], pillow)
    assert len(e2) == 1 and e2[0][0] == 3 and "clip_12.png" in e2[0][1] and "PNG decode failed" in e2[0][1]
    assert torch.isnan(gpu[3]).all()
    direct = sampling.GpuFrameLoader(str(tmp_path), names, device=eng.device)
    assert len(direct) == 4


def test_loader_threads_decode_at_once_on_their_own_streams():
    paths = sorted(glob.glob(os.path.join(GOLDEN, "png_*", "*.png")))
    want = {p: sampling.read_frame_bgr(p) for p in paths}
    errors, streams = [], set()

    def work(k):
        try:
            dec = pngdecode.decoder_for(0)
            streams.add(dec.stream.cuda_stream)
            for r in range(3):
                order = paths[k::4] + paths[:k]
                got = dec.decode(order)
                got = got if isinstance(got, list) else list(got)
                for p, g in zip(order, got):
                    if not np.array_equal(g.cpu().numpy(), want[p]):
                        errors.append((k, r, p))
        except Exception as e:          # noqa: BLE001
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors and len(streams) == 4
