"""CPU checks of the PNG path's host half: the test corpus writer (tests/png_corpus.py) against Pillow, and the container
parser (relax_vqa_amd/png.py): chunk walk, CRC failure, missing IEND, and which files the GPU decoder takes."""
import io
import os
import struct
import sys
import zlib

import numpy as np
import pytest
from PIL import Image

import relax_vqa_amd  # noqa: F401
from relax_vqa_amd import png

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_corpus  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _pillow_bgr(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1]


def test_corpus_writer_round_trips_through_pillow():
    corpus = png_corpus.corpus()
    seen_filters, seen_strategies, seen_ct, seen_w = set(), set(), set(), set()
    for name, data, want in corpus:
        assert np.array_equal(_pillow_bgr(data), want), name
        info = png.parse(data, name)
        seen_ct.add(info.color_type)
        seen_w.add(info.width)
        seen_filters.add(name.split("_f")[1].split("_")[0])
        seen_strategies.add(name.replace("tall_", "").split("_")[0])
    assert seen_filters == {"0", "1", "2", "3", "4", "mixed"}
    assert seen_strategies == {s for s, _, _ in png_corpus.STRATEGIES}
    assert seen_ct == {0, 2, 6} and {1, 3, 17, 224, 960, 1920} <= seen_w


def test_parse_walks_chunks_and_joins_idat():
    img = png_corpus.image(5, 17, 3, seed=1)
    raw = png_corpus.filter_rows(img.reshape(5, 51), 3, [0] * 5)
    z = png_corpus.compress(raw)
    data = png_corpus.container(z, 17, 5, 2, splits=[1, 2, 3, 10], ancillary=True)
    info = png.parse(data)
    assert (info.width, info.height, info.bit_depth, info.color_type, info.interlace) == (17, 5, 8, 2, 0)
    assert info.zdata == z and info.channels == 3 and info.shape == (5, 17, 3)
    assert zlib.decompress(info.zdata) == raw


def test_parse_rejects_crc_failure_and_missing_iend():
    data = bytearray(png_corpus.encode(png_corpus.image(4, 4, 3, 2), 2, 0, 6, zlib.Z_DEFAULT_STRATEGY))
    at = data.index(b"IDAT") + 6
    bad = bytearray(data)
    bad[at] ^= 0x40
    with pytest.raises(png.PngError, match="CRC mismatch in chunk 'IDAT'"):
        png.parse(bytes(bad), "x.png")
    with pytest.raises(png.PngError, match="no IEND"):
        png.parse(bytes(data[:-12]), "x.png")
    with pytest.raises(png.PngError, match="runs past the end"):
        png.parse(bytes(data[:-6]), "x.png")
    with pytest.raises(png.PngError, match="bad signature"):
        png.parse(b"GIF89a" + bytes(data[6:]), "x.png")
    no_idat = png_corpus.SIG + png_corpus.chunk(b"IHDR", struct.pack(">IIBBBBB", 4, 4, 8, 2, 0, 0, 0)) + png_corpus.chunk(b"IEND", b"")
    with pytest.raises(png.PngError, match="no IDAT"):
        png.parse(no_idat)


def _pillow_png(mode, size=(9, 5), **kw):
    im = Image.new(mode, size)
    if mode == "P":
        im.putpalette([i % 256 for i in range(768)])
    buf = io.BytesIO()
    im.save(buf, format="PNG", **kw)
    return buf.getvalue()


def test_fallback_decision_per_format():
    gpu = {"L": 1, "RGB": 3, "RGBA": 4}
    for mode, c in gpu.items():
        assert png.parse(_pillow_png(mode)).channels == c, mode
    for mode in ("P", "LA", "I;16", "1"):
        assert png.parse(_pillow_png(mode)).channels is None, mode
    z = png_corpus.compress(b"\0" * 20)
    assert png.parse(png_corpus.container(z, 3, 4, 2, interlace=1)).channels is None                  # Adam7
    assert png.parse(png_corpus.container(z, 3, 4, 2, bit_depth=16)).channels is None                 # 16-bit RGB
    assert png.parse(png_corpus.container(z, 5462, 1, 2)).channels is None                            # row wider than 16 KiB
    assert png.parse(png_corpus.container(z, 5461, 1, 2)).channels == 3


def test_golden_frames_parse_as_the_issue_describes():
    info = png.parse(open(os.path.join(GOLDEN, "png_5636101558_3", "5636101558_3.png"), "rb").read())
    assert (info.width, info.height, info.channels) == (960, 540, 3) and info.zdata[:2] == b"\x78\x9c"
