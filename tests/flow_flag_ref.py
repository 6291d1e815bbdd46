"""The definitions of the two flag bits of relax_optical_flow_flags (csrc/flow.hip: gauss_solve_any, resize_area_f32x2), in numpy, built from
oracle/flow_ref.py's own pieces (pyramid_levels, gaussian_blur, resize_linear, poly_exp, update_matrices, update_flow_blur): TEST SUPPORT, not
product.  farneback_flags re-states flow_ref.farneback's loop with two hooks:

  flags & 256 (OPTFLOW_FARNEBACK_GAUSSIAN): update_flow_blur becomes update_flow_gauss - the separable window gauss_window(winsize) over the
      five planes of M with replicated rows and columns, then update_flow_blur's 2 x 2 solve in double with the regulariser 1e-3 (no
      1 / winsize^2: the taps sum to 1).  All 2 m + 1 taps are used.
  flags & 4 (OPTFLOW_USE_INITIAL_FLOW): at the coarsest level used the zero field becomes resize_area(init, h, w) * (float)scale; finer levels
      are unchanged.

Nothing here can run OpenCV: both modes are pinned to THESE formulas and to float64, not to an OpenCV build.  What they are checked against
instead (tests/test_flow_flags_cpu.py): scipy.ndimage.correlate1d(mode='nearest') on the same taps, and exact area integration."""
import math

import numpy as np

from oracle import flow_ref

F32 = np.float32
GAUSSIAN, USE_INITIAL = 256, 4


def gauss_window(winsize):
    """float32 [m + 1], m = winsize // 2: k[0] = 1, k[i] = (float)exp(-i*i / (2 sigma^2)) with sigma = 0.3 m, s = 1 / (1 + 2 sum k[1:]) in
    double, k[i] = (float)(k[i] * s)."""
    m = winsize // 2
    sigma = 0.3 * m
    k = np.ones(m + 1, dtype=F32)
    for i in range(1, m + 1):
        k[i] = F32(math.exp(-i * i / (2 * sigma * sigma)))
    s = 1.0 / (1.0 + 2.0 * float(k[1:].astype(np.float64).sum()))
    return (k.astype(np.float64) * s).astype(F32)


def gauss_window_planes(M, winsize, dtype=F32):
    """The window over M [h, w, C]: rows, then columns, replicated borders -> dtype [h, w, C] (float32: the passes in float; float64: in double)."""
    k = gauss_window(winsize).astype(dtype)
    m = winsize // 2
    M = M.astype(dtype)
    h, w = M.shape[:2]
    ys, xs = np.arange(h), np.arange(w)
    v = M * k[0]
    for i in range(1, m + 1):
        v = v + (M[np.minimum(ys + i, h - 1)] + M[np.maximum(ys - i, 0)]) * k[i]
    out = v * k[0]
    for i in range(1, m + 1):
        out = out + (v[:, np.minimum(xs + i, w - 1)] + v[:, np.maximum(xs - i, 0)]) * k[i]
    return out


def update_flow_gauss(M, winsize=15, dtype=F32):
    """FarnebackUpdateFlow_GaussianBlur as stated above -> flow [h, w, 2]."""
    b = gauss_window_planes(M, winsize, dtype).astype(np.float64)
    g11, g12, g22, h1, h2 = (b[..., i] for i in range(5))
    idet = 1.0 / (g11 * g22 - g12 * g12 + 1e-3)
    flow = np.empty(M.shape[:2] + (2,), dtype=dtype)
    flow[..., 0] = (g11 * h2 - g12 * h1) * idet
    flow[..., 1] = (g22 * h1 - g12 * h2) * idet
    return flow


def area_table(src, dst):
    """cv::resize(INTER_AREA)'s table for one axis -> float64 [dst, src] (a dense matrix: row d holds cell d's weights).  S = src / dst; cell d
    covers [d S, d S + S), cw = min(S, src - d S); full pixels ceil(d S) .. min(floor(d S + S), src - 1) exclusive at 1 / cw, the partial pixels
    either side where their overlap exceeds 1e-3."""
    S = src / dst
    A = np.zeros((dst, src))
    for d in range(dst):
        f1 = d * S
        f2 = f1 + S
        cw = min(S, src - f1)
        s1, s2 = math.ceil(f1), math.floor(f2)
        s2 = min(s2, src - 1)
        s1 = min(s1, s2)
        if s1 - f1 > 1e-3:
            A[d, s1 - 1] = (s1 - f1) / cw
        for sx in range(s1, s2):
            A[d, sx] = 1.0 / cw
        if f2 - s2 > 1e-3:
            A[d, s2] = min(f2 - s2, 1.0, cw) / cw
    return A


def area_table_sparse(src, dst):
    """area_table in the layout of relax_flow_area_table: (first int32 [dst], count int32 [dst], weights float64 [dst, src // dst + 2])."""
    A = area_table(src, dst)
    taps = src // dst + 2
    first, count, weights = np.zeros(dst, np.int32), np.zeros(dst, np.int32), np.zeros((dst, taps))
    for d in range(dst):
        nz = np.nonzero(A[d])[0]
        first[d], count[d] = nz[0], nz[-1] - nz[0] + 1
        weights[d, :count[d]] = A[d, nz[0]:nz[-1] + 1]
    return first, count, weights


def area_integration_matrix(src, dst):
    """Area integration as it reads: entry (d, s) = |[d S, d S + S) intersected with [s, s + 1)| / S with S = src / dst, in float64 (no
    threshold, no special cases)."""
    S = src / dst
    d = np.arange(dst, dtype=np.float64)[:, None]
    s = np.arange(src, dtype=np.float64)[None, :]
    return np.maximum(np.minimum(d * S + S, s + 1) - np.maximum(d * S, s), 0) / S


def exact_area_matrix(src, dst):
    """The same from integer arithmetic, one rounding per entry: overlap = (min((d + 1) src, (s + 1) dst) - max(d src, s dst)) / dst, over S.
    (d * S in double, which both the table and area_integration_matrix start from, is itself off by up to src * 2^-53.)"""
    d = np.arange(dst, dtype=np.int64)[:, None]
    s = np.arange(src, dtype=np.int64)[None, :]
    ov = np.minimum((d + 1) * src, (s + 1) * dst) - np.maximum(d * src, s * dst)
    return np.maximum(ov, 0) / float(src)


def resize_area(img, h, w):
    """cv::resize(img, (w, h), INTER_AREA) of [H, W, C] in float64: rows, then columns."""
    H, W = img.shape[:2]
    Ay, Ax = area_table(H, h), area_table(W, w)
    return np.einsum("yY,YXc,xX->yxc", Ay, img.astype(np.float64), Ax, optimize=True)


def initial_level(init, pyr_scale, levels, dtype=F32):
    """What flags & 4 puts in place of the zero field: resize_area(init, h, w) * (float)scale at the coarsest level used."""
    H, W = init.shape[:2]
    k = flow_ref.pyramid_levels(H, W, pyr_scale, levels)
    scale = pyr_scale ** k
    h, w = flow_ref.cv_round(H * scale), flow_ref.cv_round(W * scale)
    return (resize_area(init, h, w).astype(dtype) * dtype(F32(scale))).astype(dtype)


def farneback_flags(prev_gray, next_gray, pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2, flags=0, init=None,
                    dtype=F32):
    """flow_ref.farneback's loop with the two hooks; flags 0 and init None: the same operations as flow_ref.farneback."""
    assert flags & ~(GAUSSIAN | USE_INITIAL) == 0 and (init is not None) == bool(flags & USE_INITIAL)
    update_flow = update_flow_gauss if flags & GAUSSIAN else flow_ref.update_flow_blur
    h0, w0 = prev_gray.shape
    levels = flow_ref.pyramid_levels(h0, w0, pyr_scale, levels)
    imgs = [prev_gray.astype(dtype), next_gray.astype(dtype)]
    prev_flow = None
    for k in range(levels, -1, -1):
        scale = pyr_scale ** k
        sigma = (1.0 / scale - 1) * 0.5
        smooth = max(flow_ref.cv_round(sigma * 5) | 1, 3)
        w, h = flow_ref.cv_round(w0 * scale), flow_ref.cv_round(h0 * scale)
        if prev_flow is None and init is not None:
            flow = (resize_area(init, h, w).astype(dtype) * dtype(F32(scale))).astype(dtype)
        elif prev_flow is None:
            flow = np.zeros((h, w, 2), dtype=dtype)
        else:
            flow = flow_ref.resize_linear(prev_flow, h, w, dtype) * dtype(1.0 / pyr_scale)
        R = [flow_ref.poly_exp(flow_ref.resize_linear(flow_ref.gaussian_blur(im, smooth, sigma, dtype), h, w, dtype), poly_n, poly_sigma, dtype)
             for im in imgs]
        M = flow_ref.update_matrices(R[0], R[1], flow, dtype)
        for i in range(iterations):
            flow = update_flow(M, winsize, dtype)
            if i < iterations - 1:
                M = flow_ref.update_matrices(R[0], R[1], flow, dtype)
        prev_flow = flow
    return prev_flow
