"""Run INSIDE a subprocess with libasan preloaded (tests/test_png_decode_sanitized.py): decodes the test corpus and the
malformed streams of tests/png_corpus.py through the decode core of csrc/png_inflate.h built as one-lane host code under
-fsanitize=address,undefined (librelax_png_san.so).  Inputs and outputs sit in malloc'd buffers of exactly their size, so a
read or write one byte outside them is a sanitizer report.  Any report aborts the process."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import relax_vqa_amd  # noqa: E402,F401
from relax_vqa_amd import png  # noqa: E402
import png_corpus  # noqa: E402

lib = C.CDLL(os.path.join(ROOT, "relax-vqa_amd", "csrc", "librelax_png_san.so"))
lib.relax_png_decode_host.restype = C.c_int
lib.relax_png_decode_host.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64]
libc = C.CDLL(None)
libc.malloc.restype = C.c_void_p
libc.malloc.argtypes = [C.c_size_t]
libc.free.argtypes = [C.c_void_p]


def decode(z, H, W, Ch):
    zin = libc.malloc(max(len(z), 1))
    C.memmove(zin, z, len(z))
    n = H * W * 3
    out = libc.malloc(n)
    try:
        st = lib.relax_png_decode_host(zin if z else None, len(z), H, W, Ch, out, n)
        img = np.frombuffer(C.string_at(out, n), np.uint8).reshape(H, W, 3).copy() if st == 0 else None
    finally:
        libc.free(zin)
        libc.free(out)
    return st, img


n_ok = 0
for name, data, want in png_corpus.corpus():
    info = png.parse(data, name)
    st, got = decode(info.zdata, info.height, info.width, info.channels)
    assert st == 0, (name, st, png.status_message(st))
    assert np.array_equal(got, want), name
    n_ok += 1
for case in png_corpus.malformed():
    name, z, H, W, Ch, want = case
    st, _ = decode(z, H, W, Ch)
    assert st == want, (name, st, png.status_message(st), want)
    n_ok += 1
print(f"PNG_DECODE_SANITIZED_OK {n_ok}")
