"""Inputs, references and input conditions of the content-level optical-flow checks (csrc/flow.hip), shared by
tests/test_flow_cases_cpu.py, tests/test_gpu_flow_content.py and tools/flow_content_parity.py.

Every other flow parity test moves a sum of low-frequency sinusoids by 1 to 3 pixels with np.roll: the warp of FarnebackUpdateMatrices
then leaves the frame only inside the 5-pixel border band, where OpenCV's table scales every term by 0.14 to 0.4472 per axis, and most
flow vectors point into one hue sector.  The pairs here move 9 to 17 pixels (new content enters the frame: both frames are crops of one
larger canvas), rotate and zoom (flow vectors in every direction), carry a motion boundary, noise, hard 0 / 255 edges and saturated flat
regions.  What each listed case must reach is asserted on the CPU (tests/test_flow_cases_cpu.py); the GPU is compared with the oracle in
float64, in units of the float32 oracle's own distance from it."""
import functools
import json
import os

import numpy as np

from oracle import flow_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY_JSON = os.path.join(ROOT, "profiles", "flow_content_parity.json")
PARITY_CAP = 8.0      # the cap of tests/vit_patch8_cases.py: a ratio above it is a bug, not a gate

MARGIN = 48           # canvas pixels beyond the frame on every side: the largest motion below stays well inside
SIZES = [(97, 131), (256, 264)]     # two levels, odd pixel count, the general kernels | four levels, pyramid_fused, 16-byte paths, two bands
KINDS = ["smooth", "noise", "steps", "sat"]
SHIFTS = [("shift", 9, -6), ("shift", -17, 12)]
ROTZOOMS = [("rotzoom", 4.0, 1.05), ("rotzoom", -8.0, 0.93)]
OCCLUSION = ("occlusion",)
NEW_CONTENT = ("new_content",)     # the second frame shares nothing with the first (degenerate: no correspondence)


# ---- textures ----------------------------------------------------------------------------------------------------
def texture(kind, h, w, seed):
    """float64 [h + 2 MARGIN, w + 2 MARGIN, 3], values meant for [0, 255] (clipped when a frame is cut)."""
    g = np.random.default_rng(seed)
    H, W = h + 2 * MARGIN, w + 2 * MARGIN
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    base = np.zeros((H, W, 3))
    for _ in range(12):
        fx, fy, ph = g.uniform(0.01, 0.12), g.uniform(0.01, 0.12), g.uniform(0, 6.28, 3)
        for c in range(3):
            base[..., c] += g.uniform(10, 30) * np.sin(xx * fx + yy * fy + ph[c])
    if kind == "smooth":
        return base + 128
    if kind == "noise":
        return base + 128 + g.normal(0.0, 20.0, base.shape)
    if kind == "sat":
        return 4 * base + 128          # clipped to large flat regions of 0 and 255
    if kind == "steps":                # hard edges: blocks 7 wide and 5 high, each 0 or 255
        bits = g.integers(0, 2, ((H + 4) // 5, (W + 6) // 7))
        blocks = np.repeat(np.repeat(bits, 5, axis=0), 7, axis=1)[:H, :W]
        return np.repeat(blocks[..., None] * 255.0, 3, axis=2)
    raise ValueError(kind)


def _u8(a):
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def _crop(canvas, h, w, dx=0, dy=0):
    """The frame whose content has moved by (dx, dy) against the centred crop."""
    return canvas[MARGIN - dy:MARGIN - dy + h, MARGIN - dx:MARGIN - dx + w]


def _rotzoom(canvas, h, w, deg, zoom):
    """The centred crop rotated by deg and scaled by zoom about the frame centre, bilinear."""
    t = np.deg2rad(deg)
    cy, cx = MARGIN + (h - 1) / 2.0, MARGIN + (w - 1) / 2.0
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    u, v = xx + MARGIN - cx, yy + MARGIN - cy
    sx = cx + (np.cos(t) * u + np.sin(t) * v) / zoom      # where the output pixel comes from
    sy = cy + (-np.sin(t) * u + np.cos(t) * v) / zoom
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    assert x0.min() >= 0 and y0.min() >= 0 and x0.max() < canvas.shape[1] - 1 and y0.max() < canvas.shape[0] - 1
    ax, ay = (sx - x0)[..., None], (sy - y0)[..., None]
    return ((1 - ay) * ((1 - ax) * canvas[y0, x0] + ax * canvas[y0, x0 + 1]) +
            ay * ((1 - ax) * canvas[y0 + 1, x0] + ax * canvas[y0 + 1, x0 + 1]))


def make_pair(case):
    """case = (h, w, kind, motion, seed) -> two uint8 BGR frames [h, w, 3]."""
    h, w, kind, motion, seed = case
    canvas = np.clip(texture(kind, h, w, seed), 0, 255)
    a = _crop(canvas, h, w)
    if motion[0] == "shift":
        b = _crop(canvas, h, w, motion[1], motion[2])
    elif motion[0] == "rotzoom":
        b = _rotzoom(canvas, h, w, motion[1], motion[2])
    elif motion[0] == "occlusion":       # the background moves (-3, +2); a centred rectangle of a second texture moves (+7, -4) over it
        fg = np.clip(texture(kind, h, w, seed + 1000), 0, 255)
        rh, rw, y0, x0 = h // 2, w // 2, h // 4, w // 4
        a = a.copy()
        a[y0:y0 + rh, x0:x0 + rw] = _crop(fg, h, w)[y0:y0 + rh, x0:x0 + rw]
        b = _crop(canvas, h, w, -3, 2).copy()
        b[y0 - 4:y0 - 4 + rh, x0 + 7:x0 + 7 + rw] = _crop(fg, h, w)[y0:y0 + rh, x0:x0 + rw]
    elif motion[0] == "new_content":
        b = _crop(np.clip(texture(kind, h, w, seed + 2000), 0, 255), h, w)
    else:
        raise ValueError(motion)
    return _u8(a), _u8(b)


# ---- the case list ---------------------------------------------------------------------------------------------------
# Every kind and every motion at both sizes, three pairs with different motions per line (one GPU call each).  What is NOT listed, and why:
#   * `smooth` under a shift: the low-frequency texture gives Farneback too little to follow 9 to 17 pixels (the flow stays under 8 px and no
#     interior warp leaves the frame, at every seed tried) - the large motions are on `noise`, `steps` and `sat`;
#   * `steps` under a shift at 97 x 131: two levels do not reach the motion (under 0.3 % of interior warps leave the frame);
#   * `steps` under the occlusion: the in-frame test of the warp flips between float32 and float64 at the hard-edged motion boundary (the
#     two oracles are 2e-2 px apart), and a pair on which the oracle does not agree with itself measures nothing.
# The seeds are the first from 0 at which the case meets tests/test_flow_cases_cpu.py's conditions with a margin.
_S0, _S1 = SHIFTS
_R0, _R1 = ROTZOOMS
_LISTED = {
    (97, 131): [
        ("smooth", _R0, 3), ("noise", _S0, 6), ("sat", OCCLUSION, 0),
        ("smooth", _R1, 1), ("noise", _S1, 0), ("smooth", OCCLUSION, 0),
        ("steps", _R0, 0), ("sat", _S0, 0), ("noise", OCCLUSION, 0),
        ("steps", _R1, 0), ("sat", _S1, 0), ("noise", _R0, 0),
    ],
    (256, 264): [
        ("smooth", _R0, 0), ("noise", _S0, 0), ("sat", OCCLUSION, 0),
        ("smooth", _R1, 0), ("steps", _S1, 0), ("smooth", OCCLUSION, 0),
        ("steps", _R0, 0), ("sat", _S0, 7), ("noise", OCCLUSION, 0),
        ("sat", _R1, 3), ("noise", _S1, 0), ("steps", _S0, 0),
    ],
}
CASES = [(h, w, kind, motion, seed) for (h, w) in SIZES for (kind, motion, seed) in _LISTED[(h, w)]]
DEGENERATE = {(h, w): (h, w, "sat", NEW_CONTENT, 77) for (h, w) in SIZES}


def case_id(case):
    h, w, kind, motion, seed = case
    return f"{h}x{w}-{kind}-{motion[0]}" + "".join(f"_{v:g}" for v in motion[1:]) + f"-s{seed}"


def batches(size):
    """The listed cases of one size in calls of three pairs with different motions (the lines of _LISTED)."""
    cs = [c for c in CASES if c[:2] == tuple(size)]
    return [cs[i:i + 3] for i in range(0, len(cs), 3)]


def frames_of(cases):
    """uint8 [len(cases), 2, h, w, 3]"""
    return np.stack([np.stack(make_pair(c)) for c in cases])


# ---- references and what the inputs reach ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(case):
    """-> (the oracle's flow in float64, the oracle's flow in float32), computed once per case; do not write into them."""
    a, b = make_pair(case)
    ga, gb = flow_ref.bgr2gray(a), flow_ref.bgr2gray(b)
    f64, f32 = flow_ref.farneback(ga, gb, dtype=np.float64), flow_ref.farneback(ga, gb)
    f64.setflags(write=False)
    f32.setflags(write=False)
    return f64, f32


def interior_out_of_frame_share(flow):
    """Share of the pixels more than 5 px from every edge (outside the band OpenCV's border table scales down) whose displaced position
    leaves [0, w - 1) x [0, h - 1): where FarnebackUpdateMatrices drops the second frame's terms at full weight."""
    h, w = flow.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w]
    x1, y1 = np.floor(xx + flow[..., 0]), np.floor(yy + flow[..., 1])
    out = ~((x1 >= 0) & (x1 < w - 1) & (y1 >= 0) & (y1 < h - 1))
    return float(out[6:h - 6, 6:w - 6].mean())


def hue_sector_shares(flow):
    """Share of pixels in each of the six 60-degree sectors of the flow's direction (the HSV -> BGR branch flow_to_rgb takes)."""
    ang = flow_ref.fast_atan2_deg(flow[..., 1].astype(np.float32), flow[..., 0].astype(np.float32))
    sector = np.floor(ang / 60.0).astype(np.int64) % 6
    return [float((sector == s).mean()) for s in range(6)]


def coverage_of_flow(flow):
    return {"max_flow": float(np.abs(flow).max()), "interior_out_of_frame": interior_out_of_frame_share(flow),
            "hue_sectors": hue_sector_shares(flow), "levels": flow_ref.pyramid_levels(*flow.shape[:2]) + 1}


def coverage(case):
    """What the float32 oracle's flow of the case reaches: max |flow|, interior out-of-frame share, hue-sector shares, pyramid levels."""
    return coverage_of_flow(reference(case)[1])


# ---- deliberately wrong matrix updates (the sensitivity check) ---------------------------------------------------------------
WRONG = ["r6_quarter", "r4_half", "r2_kept", "x_le", "y_le", "trunc"]


def wrong_update_matrices(bug):
    """oracle.flow_ref.update_matrices with one mistake a kernel could make (bug=None: none - bit-equal to the oracle's, which
    tests/test_flow_cases_cpu.py asserts).  For flow_ref.farneback(update_matrices=...)."""
    def f(R0, R1, flow, dtype=np.float32):
        h, w = flow.shape[:2]
        border = np.array(flow_ref._BORDER, dtype=dtype)
        xs = np.arange(w, dtype=dtype)[None, :]
        ys = np.arange(h, dtype=dtype)[:, None]
        dx, dy = flow[..., 0], flow[..., 1]
        fx, fy = xs + dx, ys + dy
        rnd = np.trunc if bug == "trunc" else np.floor
        x1, y1 = rnd(fx).astype(np.int64), rnd(fy).astype(np.int64)
        fx, fy = (fx - x1).astype(dtype), (fy - y1).astype(dtype)
        ok = (x1 >= 0) & (x1 < (w if bug == "x_le" else w - 1)) & (y1 >= 0) & (y1 < (h if bug == "y_le" else h - 1))
        xc, yc = np.clip(x1, 0, w - 2), np.clip(y1, 0, h - 2)
        a00, a01, a10, a11 = (1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy
        samp = (a00[..., None] * R1[yc, xc] + a01[..., None] * R1[yc, xc + 1] +
                a10[..., None] * R1[yc + 1, xc] + a11[..., None] * R1[yc + 1, xc + 1]).astype(dtype)
        r2 = samp[..., 0] if bug == "r2_kept" else np.where(ok, samp[..., 0], dtype(0))
        r3 = np.where(ok, samp[..., 1], dtype(0))
        r4 = np.where(ok, (R0[..., 2] + samp[..., 2]) * dtype(0.5), R0[..., 2] * dtype(0.5) if bug == "r4_half" else R0[..., 2])
        r5 = np.where(ok, (R0[..., 3] + samp[..., 3]) * dtype(0.5), R0[..., 3])
        r6 = np.where(ok, (R0[..., 4] + samp[..., 4]) * dtype(0.25), R0[..., 4] * dtype(0.25 if bug == "r6_quarter" else 0.5))
        r2 = (R0[..., 0] - r2) * dtype(0.5)
        r3 = (R0[..., 1] - r3) * dtype(0.5)
        r2 = r2 + r4 * dy + r6 * dx
        r3 = r3 + r6 * dy + r5 * dx
        sx = np.ones(w, dtype=dtype)
        sy = np.ones(h, dtype=dtype)
        for i in range(min(5, w)):
            sx[i] *= border[i]
            sx[w - 1 - i] *= border[i]
        for i in range(min(5, h)):
            sy[i] *= border[i]
            sy[h - 1 - i] *= border[i]
        scale = (sy[:, None] * sx[None, :]).astype(dtype)
        r2, r3, r4, r5, r6 = (v * scale for v in (r2, r3, r4, r5, r6))
        M = np.empty((h, w, 5), dtype=dtype)
        M[..., 0] = r4 * r4 + r6 * r6
        M[..., 1] = (r4 + r5) * r6
        M[..., 2] = r5 * r5 + r6 * r6
        M[..., 3] = r4 * r2 + r6 * r3
        M[..., 4] = r6 * r2 + r5 * r3
        return M
    return f


# ---- parity ------------------------------------------------------------------------------------------------------------
def parity_ratio(got, ref64, ref32):
    """How far `got` is from the float64 oracle, in units of the float32 oracle's own distance from it: the larger of the mean and the max
    ratio (tests/vit_patch8_cases.parity_ratio's rule)."""
    e = np.abs(np.asarray(got, dtype=np.float64) - ref64)
    c = np.abs(ref32.astype(np.float64) - ref64)
    return max(float(e.mean() / c.mean()), float(e.max() / c.max()))


def parity_gate():
    """The next power of two above the worst ratio recorded in profiles/flow_content_parity.json (tools/flow_content_parity.py measures it
    on the GPU), capped at PARITY_CAP."""
    with open(PARITY_JSON) as f:
        ratio = float(json.load(f)["flow_vs_oracle_fp32"]["worst_ratio"])
    gate = 1.0
    while gate <= ratio:
        gate *= 2.0
    return min(gate, PARITY_CAP)


# ---- flow_to_rgb on a field that hits every boundary -----------------------------------------------------------------------
MAGNITUDES = np.geomspace(1e-3, 64.0, 8).astype(np.float32)


def boundary_vectors():
    """float32 [N, 2]: the exact axis and diagonal vectors, the vector just below 360 degrees, zeros and negative zeros at every
    magnitude, then 4096 equally spaced angles x 8 magnitudes."""
    v = []
    for m in MAGNITUDES.tolist():
        v += [(m, 0), (-m, 0), (0, m), (0, -m), (m, m), (m, -m), (-m, m), (-m, -m), (m, -1e-7 * m), (m, -0.0), (-0.0, m), (-m, -0.0), (-0.0, -m)]
    v += [(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0)]
    special = np.array(v, dtype=np.float32)
    ang = np.arange(4096, dtype=np.float64) * (2 * np.pi / 4096)
    ring = np.stack([np.cos(ang)[:, None] * MAGNITUDES[None, :], np.sin(ang)[:, None] * MAGNITUDES[None, :]], axis=-1)
    return np.concatenate([special, ring.reshape(-1, 2).astype(np.float32)])


def boundary_field(pairs, h, w):
    """float32 [pairs, h, w, 2] filled from boundary_vectors(): everything when it fits, else the special vectors and every k-th of the ring
    (k odd, so that all eight magnitudes stay), a different phase per pair; the rest is zero."""
    v = boundary_vectors()
    n_special = len(v) - 4096 * 8
    out = np.zeros((pairs, h * w, 2), np.float32)
    for p in range(pairs):
        if len(v) <= h * w:
            out[p, :len(v)] = v
        else:
            k = -(-(4096 * 8) // (h * w - n_special)) | 1
            sub = np.concatenate([v[:n_special], v[n_special + p::k]])
            assert len(sub) <= h * w
            out[p, :len(sub)] = sub
    return out.reshape(pairs, h, w, 2)


def constant_magnitude_field(h, w):
    """Vectors of magnitude exactly 5 in float32 (axis vectors and 3-4-5 triangles): the magnitude range is empty."""
    v = np.array([(5, 0), (0, 5), (-5, 0), (0, -5), (3, 4), (-3, 4), (3, -4), (-3, -4), (4, 3), (-4, 3), (4, -3), (-4, -3)], np.float32)
    return v[np.arange(h * w) % len(v)].reshape(1, h, w, 2)


def visualisation_parts(flow):
    """The oracle's flow_to_rgb in steps, for one flow [h, w, 2]: (hue before truncation, V before truncation, the image)."""
    x, y = flow[..., 0], flow[..., 1]
    mag = np.sqrt(x * x + y * y).astype(np.float32)
    ang = (flow_ref.fast_atan2_deg(y, x) * np.float32(np.pi / 180)).astype(np.float32)
    hue = ang * np.float32(180) / np.float32(np.pi) / np.float32(2)
    val = flow_ref._normalize_minmax(flow_ref._normalize_minmax(mag))
    return hue, val, flow_ref.flow_to_rgb(flow)


NEAR = 1e-3       # how close to an integer a value must lie before its truncation may differ: the fp32 ulp at 180 / 255 is 1.5e-5, a few
                  # reassociated or contracted operations stay under 1e-4; ten times that, and still only ~0.4 % of the pixels qualify


def unexplained_pixels(got, flow):
    """got: uint8 [h, w, 3] from the GPU for `flow`.  -> (number of pixels that differ from the oracle's but are explained, indices of the
    pixels that are not).  A pixel is explained when it is hsv_to_bgr_u8 of (H', 255, V') with |H' - H| <= 1 (mod 180), |V' - V| <= 1, H' != H
    only where the oracle's hue lies within NEAR of an integer before truncation, V' != V only where its V does."""
    hue, val, want = visualisation_parts(flow)
    bad = np.argwhere((got != want).any(axis=-1))
    explained, unexplained = 0, []
    for y, x in bad:
        hf, vf = float(hue[y, x]), float(val[y, x])
        H, V = int(np.uint8(hf)), int(np.uint8(vf))
        hs = [H - 1, H, H + 1] if abs(hf - round(hf)) <= NEAR else [H]
        vs = [V - 1, V, V + 1] if abs(vf - round(vf)) <= NEAR else [V]
        cand = np.array([[(h_ % 180, 255, v_) for h_ in hs for v_ in vs if 0 <= v_ <= 255]], dtype=np.uint8)
        if (flow_ref.hsv_to_bgr_u8(cand)[0] == got[y, x]).all(axis=-1).any():
            explained += 1
        else:
            unexplained.append((int(y), int(x)))
    return explained, unexplained
