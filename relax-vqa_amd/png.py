"""The PNG container around the GPU decoder and encoder (csrc/png_decode.hip, csrc/png_encode.hip).  parse(): the signature,
IHDR, the IDAT payloads joined into one zlib stream, IEND, and every chunk's CRC.  build(): the file around a zlib stream.  Ancillary chunks (gAMA, cHRM, cICP, pHYs, tEXt, ...) are skipped, as
cv2.imread and the Pillow path (sampling.read_frame_bgr) ignore them.  Pure Python over chunk headers: the CRCs run in zlib."""
import struct
import zlib

SIGNATURE = b"\x89PNG\r\n\x1a\n"
MAX_ROW_BYTES = 16384           # W*C limit of the GPU decoder (the previous and the current row share its 32 KiB LDS window)
GPU_CHANNELS = {0: 1, 2: 3, 6: 4}   # colour type -> channels the GPU path decodes (gray, RGB, RGBA)


class PngError(ValueError):
    """A file that is not a well-formed PNG container."""


class PngInfo:
    __slots__ = ("width", "height", "bit_depth", "color_type", "interlace", "zdata")

    def __init__(self, width, height, bit_depth, color_type, interlace, zdata):
        self.width, self.height, self.bit_depth = width, height, bit_depth
        self.color_type, self.interlace, self.zdata = color_type, interlace, zdata

    @property
    def channels(self):
        """Channels the GPU decoder takes for this file, or None: the file is decoded on the host (16-bit, palette,
        gray + alpha, Adam7, or rows wider than the decoder's limit)."""
        c = GPU_CHANNELS.get(self.color_type)
        if c is None or self.bit_depth != 8 or self.interlace != 0 or self.width * c > MAX_ROW_BYTES:
            return None
        return c

    @property
    def shape(self):
        return (self.height, self.width, 3)


def parse(data, name="<bytes>"):
    """bytes of a PNG file -> PngInfo.  Raises PngError (naming `name`) on a bad signature, a chunk that runs past the end
    of the file, a CRC mismatch, a missing or malformed IHDR, no IDAT, or no IEND."""
    mv = memoryview(data)
    if bytes(mv[:8]) != SIGNATURE:
        raise PngError(f"{name}: not a PNG file (bad signature)")
    at, n = 8, len(mv)
    ihdr, parts, seen_iend = None, [], False
    while at < n:
        length, ctype = struct.unpack(">I4s", mv[at:at + 8]) if at + 8 <= n else (0, b"?")
        end = at + 12 + length
        if length > 0x7FFFFFFF or end > n:
            raise PngError(f"{name}: chunk {ctype!r} at byte {at} runs past the end of the file")
        body = mv[at + 8:at + 8 + length]
        (crc,) = struct.unpack(">I", mv[at + 8 + length:end])
        if zlib.crc32(body, zlib.crc32(ctype)) != crc:
            raise PngError(f"{name}: CRC mismatch in chunk {ctype.decode('latin-1')!r} at byte {at}")
        if ihdr is None and ctype != b"IHDR":
            raise PngError(f"{name}: the first chunk is {ctype!r}, not IHDR")
        if ctype == b"IHDR":
            if ihdr is not None or length != 13:
                raise PngError(f"{name}: malformed IHDR")
            ihdr = struct.unpack(">IIBBBBB", body)
        elif ctype == b"IDAT":
            parts.append(body)
        elif ctype == b"IEND":
            seen_iend = True
            break
        at = end
    if ihdr is None:
        raise PngError(f"{name}: no IHDR chunk")
    if not parts:
        raise PngError(f"{name}: no IDAT chunk")
    if not seen_iend:
        raise PngError(f"{name}: no IEND chunk (truncated file)")
    w, h, depth, ctype_, _comp, _filt, interlace = ihdr
    if w < 1 or h < 1:
        raise PngError(f"{name}: empty image {w}x{h}")
    zdata = bytes(parts[0]) if len(parts) == 1 else b"".join(parts)
    return PngInfo(w, h, depth, ctype_, interlace, zdata)


def _chunk(ctype, body):
    return struct.pack(">I", len(body)) + ctype + bytes(body) + struct.pack(">I", zlib.crc32(body, zlib.crc32(ctype)))


def build(zdata, width, height, color_type):
    """A zlib stream of filtered rows (relax_png_encode's output) -> the bytes of an 8-bit, non-interlaced PNG file: signature,
    IHDR, one IDAT, IEND.  The CRCs run on the host in zlib (a v1 choice: DESIGN.md section 8 has its measured share)."""
    if color_type not in (0, 2) or width < 1 or height < 1:
        raise PngError(f"cannot build a {width}x{height} PNG of colour type {color_type}")
    return b"".join((SIGNATURE, _chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, color_type, 0, 0, 0)),
                     _chunk(b"IDAT", zdata), _chunk(b"IEND", b"")))


def read_source(src):
    """A file path or the bytes of a file -> (name for messages, bytes)."""
    if isinstance(src, (bytes, bytearray, memoryview)):
        return "<bytes>", bytes(src)
    with open(src, "rb") as f:
        return str(src), f.read()


STATUS = {
    0: "ok",
    1: "bad arguments (geometry or buffer range)",
    2: "bad zlib header",
    3: "zlib preset dictionary",
    4: "truncated zlib stream",
    5: "reserved deflate block type 3",
    6: "stored block length check failed",
    7: "invalid Huffman code-length set",
    8: "invalid literal/length or distance code",
    9: "distance reaches before the start of the output",
    10: "inflated data longer than H*(1+W*C)",
    11: "inflated data shorter than H*(1+W*C)",
    12: "unknown PNG row filter",
    13: "Adler-32 mismatch",
    14: "encode: the output slot is shorter than the stream",
}


def status_message(code):
    return STATUS.get(int(code), f"unknown status {int(code)}")
