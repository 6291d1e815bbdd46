"""The colour table of the attention overlay (src/demo_visual.py:21: cv2.applyColorMap(.., cv2.COLORMAP_JET)).

jet is the published piecewise-linear map below (the one matplotlib's "jet" uses, matplotlib/_cm.py), sampled at 256
levels the way matplotlib's LinearSegmentedColormap samples it (level i at x = i / 255, linear between the anchors) and rounded to
uint8 as rint(255 * c) (round half to even).  OpenCV's own COLORMAP_JET table is close to it but not the same bits, so the
overlay matches the reference's colours only up to that table.  Where cv2 is installed, its exact table can be passed instead:

    lut = cv2.applyColorMap(np.arange(256, dtype=np.uint8)[:, None], cv2.COLORMAP_JET)[:, 0, :]   # uint8 [256, 3] BGR
    engine.attention_overlay(frames, positions, counts, patch_values, lut=lut)
"""
import numpy as np

# (x, value) anchors per channel; the map is continuous, so matplotlib's (x, y0, y1) triples have y0 == y1
JET_ANCHORS = {
    "red": ((0.0, 0.0), (0.35, 0.0), (0.66, 1.0), (0.89, 1.0), (1.0, 0.5)),
    "green": ((0.0, 0.0), (0.125, 0.0), (0.375, 1.0), (0.64, 1.0), (0.91, 0.0), (1.0, 0.0)),
    "blue": ((0.0, 0.5), (0.11, 1.0), (0.34, 1.0), (0.65, 0.0), (1.0, 0.0)),
}


def _channel(anchors, n):
    """matplotlib.colors._create_lookup_table(n, anchors) for a continuous map (gamma 1), in float64."""
    x = np.array([a[0] for a in anchors], dtype=np.float64) * (n - 1)
    y = np.array([a[1] for a in anchors], dtype=np.float64)
    xind = (n - 1) * np.linspace(0, 1, n)
    ind = np.searchsorted(x, xind)[1:-1]
    distance = (xind[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
    lut = np.concatenate([[y[0]], distance * (y[ind] - y[ind - 1]) + y[ind - 1], [y[-1]]])
    return np.clip(lut, 0.0, 1.0)


def jet_rgb_float(n=256):
    """float64 [n, 3] RGB in [0, 1]."""
    return np.stack([_channel(JET_ANCHORS[c], n) for c in ("red", "green", "blue")], axis=1)


def jet_lut_bgr():
    """uint8 [256, 3] BGR: rint(255 * jet), the default table of RelaxEngine.attention_overlay."""
    return np.ascontiguousarray(np.rint(jet_rgb_float(256) * 255.0)[:, ::-1]).astype(np.uint8)
