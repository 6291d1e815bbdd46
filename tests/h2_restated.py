"""numpy restatement of the two-fp16-plane format of csrc/h2.h (split2_pair, the chunk layout of a row) for the tests of the plane
outputs and plane residuals: numpy's float casts round to nearest even, as the device's conversions do, and x s - hi is exact in fp32."""
import numpy as np


def split2(x, s):
    """fp32 x, power-of-two scale(s) s (broadcast) -> (hi, lo) as uint16 bit patterns: hi = fp16(x s), lo = fp16(x s - hi)."""
    xs = (np.asarray(x, dtype=np.float32) * np.asarray(s, dtype=np.float32)).astype(np.float32)
    with np.errstate(over="ignore"):
        hi = xs.astype(np.float16)
        lo = (xs - hi.astype(np.float32)).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


def join2(hi, lo, inv):
    """(hi + lo) * inv in fp32: the value the planes stand for (exact: at most 24 bits times a power of two)."""
    return ((hi.view(np.float16).astype(np.float32) + lo.view(np.float16).astype(np.float32)) * np.asarray(inv, dtype=np.float32)).astype(np.float32)


def to_rows(hi, lo):
    """hi, lo [M, N] (N % 16 == 0) -> the stored rows [M, 2 N] uint16: per 16 values one chunk of 16 x hi, 16 x lo."""
    m, n = hi.shape
    return np.concatenate([hi.reshape(m, n // 16, 16), lo.reshape(m, n // 16, 16)], axis=2).reshape(m, 2 * n)


def from_rows(rows):
    """The inverse of to_rows: stored rows [M, 2 N] uint16 -> (hi, lo) [M, N]."""
    m, n2 = rows.shape
    c = rows.reshape(m, n2 // 32, 32)
    return c[:, :, :16].reshape(m, n2 // 2), c[:, :, 16:].reshape(m, n2 // 2)


def pow2_scale(amax, top):
    """Per entry of amax the power of two s with amax s in [2^(top-1), 2^top); 1 where amax is 0."""
    amax = np.asarray(amax, dtype=np.float64)
    e = np.frexp(np.where(amax > 0, amax, 1.0))[1]          # amax in [2^(e-1), 2^e)
    return np.where(amax > 0, np.exp2((top - e).astype(np.float64)), 1.0).astype(np.float32)
