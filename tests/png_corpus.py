"""A small PNG writer (numpy + zlib) and the decoder's test corpus, built at test time.  The writer picks each row's filter
(None, Sub, Up, Average, Paeth or a mix), the zlib settings (level 0 = stored blocks only, Z_FIXED, Z_HUFFMAN_ONLY, Z_RLE,
default, level 9) and where the zlib stream is cut into IDAT chunks (1-byte chunks included); some files carry ancillary
chunks.  `malformed()` hand-assembles broken deflate streams, each with the status the decoder must give it."""
import struct
import zlib

import numpy as np

SIG = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 6: 4}

ST_TRUNCATED, ST_BAD_BLOCK_TYPE, ST_BAD_STORED_LEN, ST_BAD_CODE_LENGTHS = 4, 5, 6, 7
ST_BAD_SYMBOL, ST_DIST_TOO_FAR, ST_TOO_LONG, ST_TOO_SHORT, ST_BAD_FILTER, ST_BAD_ADLER = 8, 9, 10, 11, 12, 13
ST_BAD_ZLIB_HEADER, ST_PRESET_DICT = 2, 3

STRATEGIES = [("stored", 0, zlib.Z_DEFAULT_STRATEGY), ("fixed", 6, zlib.Z_FIXED), ("huffman", 6, zlib.Z_HUFFMAN_ONLY),
              ("rle", 6, zlib.Z_RLE), ("default", 6, zlib.Z_DEFAULT_STRATEGY), ("best", 9, zlib.Z_DEFAULT_STRATEGY)]
FILTERS = [0, 1, 2, 3, 4, "mixed"]


def chunk(ctype, body):
    return struct.pack(">I", len(body)) + ctype + body + struct.pack(">I", zlib.crc32(body, zlib.crc32(ctype)))


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(rows, bpp, filters):
    """rows uint8 [H, W*C], filters: one type (0-4) per row -> the filtered stream bytes (filter byte + row, per row)."""
    H, n = rows.shape
    out = bytearray()
    prev = np.zeros(n, np.int32)
    for y in range(H):
        x = rows[y].astype(np.int32)
        a = np.concatenate([np.zeros(bpp, np.int32), x[:-bpp]]) if n > bpp else np.zeros(n, np.int32)
        a = a[:n]
        c = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]])[:n]
        f = int(filters[y])
        if f == 0:
            d = x
        elif f == 1:
            d = x - a
        elif f == 2:
            d = x - prev
        elif f == 3:
            d = x - ((a + prev) >> 1)
        else:
            d = x - _paeth(a, prev, c)
        out.append(f)
        out += (d & 255).astype(np.uint8).tobytes()
        prev = x
    return bytes(out)


def compress(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    return co.compress(raw) + co.flush()


def container(zdata, W, H, color_type, bit_depth=8, interlace=0, splits=None, ancillary=False):
    """A PNG file around a zlib stream; `splits`: the byte offsets where a new IDAT chunk starts."""
    out = SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, bit_depth, color_type, 0, 0, interlace))
    if ancillary:
        out += chunk(b"gAMA", struct.pack(">I", 45455)) + chunk(b"pHYs", struct.pack(">IIB", 2835, 2835, 1))
        out += chunk(b"cHRM", struct.pack(">8I", 31270, 32900, 64000, 33000, 30000, 60000, 15000, 6000))
        out += chunk(b"cICP", bytes([1, 13, 0, 1])) + chunk(b"tEXt", b"Comment\x00png_corpus")
    cuts = [0] + sorted(set(s for s in (splits or []) if 0 < s < len(zdata))) + [len(zdata)]
    for lo, hi in zip(cuts, cuts[1:]):
        out += chunk(b"IDAT", zdata[lo:hi])
    return out + chunk(b"IEND", b"")


def image(H, W, C, seed):
    """Pixels with structure (gradients, repeats) and noise, so every strategy finds matches and literals."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([(x * 7 + y * 3 + 40 * k) % 256 for k in range(C)], -1)
    noise = rng.integers(0, 256, (H, W, C))
    band = ((y // 3) % 4 == 1)[..., None]
    img = np.where(band, noise, base)
    img[:, W // 2:] = np.where(rng.random((H, W - W // 2, 1)) < 0.1, noise[:, W // 2:], img[:, W // 2:])
    return img.astype(np.uint8)


def encode(img, color_type, filt, level, strategy, splits=None, ancillary=False, seed=0):
    H, W = img.shape[:2]
    C = CHANNELS[color_type]
    rows = img.reshape(H, W * C)
    if filt == "mixed":
        filters = np.random.default_rng(seed + 7).integers(0, 5, H)
    else:
        filters = [filt] * H
    raw = filter_rows(rows, C, filters)
    return container(compress(raw, level, strategy), W, H, color_type, splits=splits, ancillary=ancillary)


def expected_bgr(img, color_type):
    if color_type == 0:
        g = img.reshape(img.shape[0], img.shape[1])
        return np.repeat(g[..., None], 3, axis=2)
    return np.ascontiguousarray(img[..., :3][..., ::-1])


SHAPES = [(1, 1), (4, 1), (1, 3), (5, 3), (9, 17), (1, 17), (12, 224), (3, 224), (6, 960), (2, 960), (3, 1920), (1, 1920)]


def corpus():
    """-> [(name, png bytes, expected BGR uint8 [H,W,3])]: every filter with every zlib setting, widths 1 to 1920, colour
    types 0 / 2 / 6, IDAT chunks cut at arbitrary offsets (some of 1 byte), some files with ancillary chunks."""
    out = []
    k = 0
    for fi, filt in enumerate(FILTERS):
        for si, (sname, level, strategy) in enumerate(STRATEGIES):
            H, W = SHAPES[(fi * 5 + si * 7) % len(SHAPES)]
            ct = (0, 2, 6)[(fi + si) % 3]
            img = image(H, W, CHANNELS[ct], seed=k)
            rng = np.random.default_rng(1000 + k)
            splits = None
            if k % 3 == 0:
                splits = list(rng.integers(1, 400, 6)) + [1, 2, 3]          # 1-byte chunks at the start, then arbitrary cuts
            elif k % 3 == 1:
                splits = list(np.cumsum(rng.integers(1, 5000, 30)))
            data = encode(img, ct, filt, level, strategy, splits=splits, ancillary=(k % 4 == 1), seed=k)
            out.append((f"{sname}_f{filt}_ct{ct}_{W}x{H}", data, expected_bgr(img, ct)))
            k += 1
    # taller images: several deflate blocks, the window ring wrapping many times
    for ct, (H, W), filt, (sname, level, strategy) in ((2, (40, 960), "mixed", STRATEGIES[4]), (6, (24, 224), 4, STRATEGIES[5]),
                                                       (0, (70, 1920), "mixed", STRATEGIES[0]), (2, (30, 1920), 4, STRATEGIES[3])):
        img = image(H, W, CHANNELS[ct], seed=k)
        data = encode(img, ct, filt, level, strategy, ancillary=True, seed=k)
        out.append((f"tall_{sname}_f{filt}_ct{ct}_{W}x{H}", data, expected_bgr(img, ct)))
        k += 1
    return out


class BitWriter:
    def __init__(self):
        self.bits = []

    def put(self, value, n):                # deflate header fields and extra bits: least significant bit first
        self.bits += [(value >> i) & 1 for i in range(n)]

    def code(self, value, n):               # Huffman codes: most significant bit first
        self.bits += [(value >> (n - 1 - i)) & 1 for i in range(n)]

    def getvalue(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + j] << j for j in range(8)) for i in range(0, len(b), 8))


ZHDR = b"\x78\x9c"


def _adler(raw):
    return struct.pack(">I", zlib.adler32(raw))


def malformed():
    """-> [(name, zlib stream, H, W, C, status)] for a 6x17 RGB image: each stream breaks one rule of zlib, deflate or PNG."""
    H, W, C = 6, 17, 3
    img = image(H, W, C, seed=99)
    raw = filter_rows(img.reshape(H, W * C), C, [0, 1, 2, 3, 4, 0])
    good = compress(raw, 6, zlib.Z_HUFFMAN_ONLY)
    cases = []
    cases.append(("truncated_mid_stream", good[:len(good) // 2], ST_TRUNCATED))
    cases.append(("truncated_in_adler", good[:-2], ST_TRUNCATED))
    cases.append(("empty", b"", ST_TRUNCATED))
    cases.append(("bad_adler", good[:-1] + bytes([good[-1] ^ 1]), ST_BAD_ADLER))
    cases.append(("too_long", compress(raw + b"\0" * 10), ST_TOO_LONG))
    cases.append(("too_short", compress(raw[:-5]), ST_TOO_SHORT))
    bad = bytearray(raw)
    bad[2 * (W * C + 1)] = 7                 # row 2's filter byte
    cases.append(("bad_filter", compress(bytes(bad)), ST_BAD_FILTER))
    cases.append(("bad_zlib_header", b"\x78\x9d" + good[2:], ST_BAD_ZLIB_HEADER))
    cases.append(("preset_dictionary", b"\x78\xbb" + good[2:], ST_PRESET_DICT))
    # dynamic block whose code-length code is over-subscribed: 19 codes of length 1
    bw = BitWriter()
    bw.put(1, 1); bw.put(2, 2); bw.put(0, 5); bw.put(0, 5); bw.put(15, 4)
    for _ in range(19):
        bw.put(1, 3)
    cases.append(("oversubscribed_code_lengths", ZHDR + bw.getvalue() + b"\0" * 16, ST_BAD_CODE_LENGTHS))
    # incomplete code-length code: two codes of length 2 (symbols 16 and 0 of the first four)
    bw = BitWriter()
    bw.put(1, 1); bw.put(2, 2); bw.put(0, 5); bw.put(0, 5); bw.put(0, 4)
    for v in (2, 0, 0, 2):
        bw.put(v, 3)
    cases.append(("incomplete_code_lengths", ZHDR + bw.getvalue() + b"\0" * 16, ST_BAD_CODE_LENGTHS))
    # fixed block that starts with a match (length 3, distance 1) before any byte exists
    bw = BitWriter()
    bw.put(1, 1); bw.put(1, 2)
    bw.code(0b0000001, 7)                    # length symbol 257
    bw.code(0, 5)                            # distance symbol 0: distance 1
    bw.code(0, 7)                            # end of block
    cases.append(("distance_before_start", ZHDR + bw.getvalue() + _adler(raw), ST_DIST_TOO_FAR))
    # fixed block: literal 'A', then a match with distance symbol 30 (not a valid distance)
    bw = BitWriter()
    bw.put(1, 1); bw.put(1, 2)
    bw.code(0x30 + 0x41, 8)
    bw.code(0b0000001, 7)
    bw.code(30, 5)
    bw.code(0, 7)
    cases.append(("invalid_distance_symbol", ZHDR + bw.getvalue() + _adler(raw), ST_BAD_SYMBOL))
    bw = BitWriter()
    bw.put(1, 1); bw.put(3, 2)
    cases.append(("reserved_block_type", ZHDR + bw.getvalue() + b"\0" * 8, ST_BAD_BLOCK_TYPE))
    cases.append(("stored_length_check", ZHDR + b"\x01" + struct.pack("<HH", 10, 10) + b"\0" * 14, ST_BAD_STORED_LEN))
    return [(name, z, H, W, C, st) for name, z, st in cases]


def malformed_png(case):
    name, z, H, W, C, st = case
    return container(z, W, H, 2)
