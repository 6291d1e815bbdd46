"""The test table of relax_optical_flow_flags (csrc/flow.hip: the Gaussian window, flags 256, and the initial flow, flags 4), shared by
tests/test_flow_flags_cpu.py, tests/test_gpu_flow_flags.py and tools/flow_flags_parity.py.  Inputs are tests/flow_cases.make_pair's on the
contents of tests/flow_param_cases.py; the reference is tests/flow_flag_ref.farneback_flags in float64 and float32 (computed once per case);
the measure is flow_cases.parity_ratio and the gate flow_param_cases.parity_gate's rule on profiles/flow_flags_parity.json.  Both modes are
pinned to the formulas of tests/flow_flag_ref.py, not to an OpenCV build."""
import functools
import json
import os

import numpy as np

from oracle import flow_ref
from tests import flow_cases as fc
from tests import flow_flag_ref as fr
from tests import flow_param_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY_JSON = os.path.join(ROOT, "profiles", "flow_flags_parity.json")

SMALL, LARGE = pc.SMALL, pc.LARGE
SMOOTH, SECOND, THIRD = pc.SMOOTH, pc.SECOND, pc.THIRD
WELL_POSED, OUTLIER_SHARE = pc.WELL_POSED, pc.OUTLIER_SHARE


def _p(*v):
    return dict(zip(pc.KEYS + ("flags",), v))


# name -> (parameters with flags, frame sizes)
SETS = {
    "gauss15": (_p(0.5, 3, 15, 3, 5, 1.2, 256), [SMALL, LARGE]),      # the literal window: the two-kernel route where flags 0 runs the fused one
    "gauss9": (_p(0.5, 1, 9, 1, 5, 1.2, 256), [SMALL]),               # narrow window, one iteration: the magnitude range on the only launch
    "gauss33": (_p(0.5, 0, 33, 5, 5, 1.2, 256), [SMALL, LARGE]),      # single level, five iterations
    "gauss63": (_p(0.5, 1, 63, 2, 5, 1.1, 256), [SMALL]),             # the widest window: the 47 KB tile; clamped rows and columns dominate
    "gauss25s08p7": (_p(0.8, 4, 25, 2, 7, 1.5, 256), [SMALL]),        # with poly_n 7 and a non-dyadic pyramid
    "init_lit": (_p(0.5, 3, 15, 3, 5, 1.2, 4), [SMALL, LARGE]),       # area resize to 48 x 66 (fractional) | 32 x 33 (exact / 8); the fused iteration
    "init_l0": (_p(0.5, 0, 15, 1, 5, 1.2, 4), [SMALL]),               # the resize is a copy
    "init_s08": (_p(0.8, 4, 21, 2, 5, 1.2, 4), [SMALL]),              # fractional tables, box_solve_any
    "init_gauss": (_p(0.6, 2, 25, 2, 5, 1.2, 260), [SMALL]),          # both bits
}
INIT_SETS = tuple(n for n, (p, _) in SETS.items() if p["flags"] & 4)
GAUSS_SETS = tuple(n for n, (p, _) in SETS.items() if p["flags"] & 256)

# What is gated where.  At a set's first size: the smooth and the noise pair, flow_cases.parity_ratio.  At the second size:
#   gauss15 - the float32 reference is itself ill-posed on the smooth pair at 256 x 264 (max |fp32 - fp64| 5.2e-3, 8.7e-4 of the components past
#             1e-3: too close to OUTLIER_SHARE) - the noise pair in full and the MEAN term alone of the smooth one;
#   gauss33, init_lit - the smooth pair.
# (kind: "full" = parity_ratio, "mean" = its mean term)
def gated_cases():
    out = []
    for name, (_, sizes) in SETS.items():
        out.append((name, pc.pair_case(sizes[0], SMOOTH), "full"))
        out.append((name, pc.pair_case(sizes[0], SECOND), "full"))
        if len(sizes) > 1 and name == "gauss15":
            out.append((name, pc.pair_case(sizes[1], SECOND), "full"))
            out.append((name, pc.pair_case(sizes[1], SMOOTH), "mean"))
        elif len(sizes) > 1:
            out.append((name, pc.pair_case(sizes[1], SMOOTH), "full"))
    return out


def gated_id(item):
    return f"{item[0]}-{fc.case_id(item[1])}" + ("-mean" if item[2] == "mean" else "")


def set_sizes():
    return [(name, size) for name, (_, sizes) in SETS.items() for size in sizes]


def batch_of(name, size):
    """The pairs of one GPU call: three different contents."""
    return [pc.pair_case(size, SMOOTH), pc.pair_case(size, SECOND), pc.pair_case(size, THIRD)]


# ---- the initial fields ------------------------------------------------------------------------------------------------------------------
# Deterministic and smooth: a base vector plus sines of AMPLITUDE pixels or more, a different phase per pair.  The base is near the shift of the
# gated contents (fc.SHIFTS[0] = (9, -6)) but not on it, so that the field is neither the answer nor noise.  What a field must do is asserted on
# the CPU (tests/test_flow_flags_cpu.py): for every init_* set at least one gated case has a float64 reference that differs from the same
# parameters without the initial flow by a mean of INIT_EFFECT px or more.  Measured on the noise pair (the smooth one converges every field
# away: under 0.002 px, 0.24 for init_l0): init_lit 2.0, init_l0 5.0, init_gauss 0.41, init_s08 3.2.  init_s08 and init_gauss needed stronger
# fields than +- 0.75 px around (6, -4) or (9, -6) - five levels of two 21-pixel iterations converge those away (0.006 px and less; init_gauss
# 0.025) - so theirs start further from the motion.
AMPLITUDE = 0.75
INIT_EFFECT = 0.1
FIELDS = {     # name -> (base x, base y, amplitude)
    "init_lit": (6.0, -4.0, 0.75),
    "init_l0": (6.0, -4.0, 0.75),
    "init_s08": (25.0, -20.0, 3.0),
    "init_gauss": (15.0, -12.0, 1.0),
}


def initial_field(name, case):
    """float32 [h, w, 2] for one pair of a set"""
    h, w = case[:2]
    bx, by, amp = FIELDS[name]
    assert amp >= AMPLITUDE
    phase = 0.7 * case[4] + (1.3 if case[2] == "noise" else 0.0)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    fx = bx + amp * np.sin(2 * np.pi * (1.5 * xx / w + 0.5 * yy / h) + phase)
    fy = by + amp * np.cos(2 * np.pi * (1.0 * xx / w - 1.25 * yy / h) + phase)
    return np.stack([fx, fy], axis=-1).astype(np.float32)


def initial_fields(name, cases):
    """float32 [len(cases), h, w, 2], or None for a set without the bit"""
    if name not in INIT_SETS:
        return None
    return np.stack([initial_field(name, c) for c in cases])


# ---- references --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(items, case, init_name):
    a, b = fc.make_pair(case)
    ga, gb = flow_ref.bgr2gray(a), flow_ref.bgr2gray(b)
    params = dict(items)
    init = None if init_name is None else initial_field(init_name, case)
    f64 = fr.farneback_flags(ga, gb, init=None if init is None else init.astype(np.float64), dtype=np.float64, **params)
    f32 = fr.farneback_flags(ga, gb, init=init, **params)
    f64.setflags(write=False)
    f32.setflags(write=False)
    return f64, f32


def reference(name, case, **other):
    """-> (float64 reference, float32 reference) of a set's pair, computed once; `other` replaces parameters (flags=0: the same six without
    the modes, and then without the initial field).  Do not write into them."""
    params = {**SETS[name][0], **other}
    return _reference(tuple(sorted(params.items())), case, name if params["flags"] & 4 else None)


def case_ratio(kind, got, ref64, ref32):
    mean_r, _ = pc.parity_terms(got, ref64, ref32)
    return mean_r if kind == "mean" else fc.parity_ratio(got, ref64, ref32)


def parity_gate():
    """flow_param_cases.parity_gate's rule on this record: the next power of two above the worst ratio recorded in
    profiles/flow_flags_parity.json (tools/flow_flags_parity.py measures it on the GPU), capped at flow_cases.PARITY_CAP."""
    with open(PARITY_JSON) as f:
        ratio = float(json.load(f)["flow_vs_reference_fp32"]["worst_ratio"])
    gate = 1.0
    while gate <= ratio:
        gate *= 2.0
    return min(gate, fc.PARITY_CAP)


# ---- the edges of gauss_solve_any ---------------------------------------------------------------------------------------------------------
TILE_W, TILE_H = 64, 32          # csrc/flow.hip: GS_TW, GS_TH


def edge_cases():
    """(winsize, h, w) on the noise pair, flags 256, one level, two iterations: widths one column either side of the tile width and 2 x tile + 1,
    heights 2 winsize +- 1 and 16 (shorter than the window)."""
    out = []
    for ws in (9, 63):
        for w in (TILE_W - 1, TILE_W + 1, 2 * TILE_W + 1):
            out.append((ws, 2 * ws + 1, w))
        out.append((ws, 2 * ws - 1, TILE_W))
        out.append((ws, 16, TILE_W + 1))
    return out


def edge_params(ws):
    return _p(0.5, 0, ws, 2, 5, 1.2, 256)


@functools.lru_cache(maxsize=None)
def edge_reference(ws, h, w):
    case = pc.pair_case((h, w), SECOND)
    return _reference(tuple(sorted(edge_params(ws).items())), case, None)
