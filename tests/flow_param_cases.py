"""Parameter sets, inputs and references of the optical-flow checks with OpenCV's parameters as arguments (relax_optical_flow_ex,
csrc/flow.hip), shared by tests/test_flow_params_cpu.py, tests/test_gpu_flow_params.py, tools/flow_params_parity.py and
tools/flow_params_bench.py.  Inputs are tests/flow_cases.make_pair's; the reference is oracle/flow_ref.farneback with the same six
parameters, in float64 and in float32 (computed once per case).

The sets below move ONE parameter at a time away from the literal set.  tests/flow_param_space.py holds the parameters in combination
(every pyr_scale with windows under, at and over 15; poly_n 7 and pyr_scale != 0.5 with box_solve_any; pyramid_fused with box_solve_any; the
sampled pyramid kernels at 0.6, 0.7 and 0.8; nine levels at 0.95; ten iterations; widths and heights at the band and segment edges) and uses
this module's contents, references, parity terms and gate.  Neither covers the 39- and 79-tap wide kernels in combination (deep4 / deep5
here run them with the literal window and poly_n), 2160p frames, or poly_sigma outside 1.1 .. 2.0."""
import functools
import json
import os

import numpy as np

from oracle import flow_ref
from tests import flow_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY_JSON = os.path.join(ROOT, "profiles", "flow_params_parity.json")

KEYS = ("pyr_scale", "levels", "winsize", "iterations", "poly_n", "poly_sigma")
LITERAL = dict(pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2)
SMALL, LARGE = (97, 131), (256, 264)


def _p(*v):
    return dict(zip(KEYS, v))


# name -> (parameters, frame sizes): each set at the smallest frame where its kernels can still go wrong
SETS = {
    "literal": (_p(0.5, 3, 15, 3, 5, 1.2), [SMALL, LARGE]),     # _ex == the old entry, bits
    "poly7": (_p(0.5, 3, 15, 3, 7, 1.5), [SMALL, LARGE]),       # 15-row ring, 242-column band, another sigma
    "win9": (_p(0.5, 1, 9, 1, 5, 1.2), [SMALL]),                # narrow window, one iteration, two levels
    "win25": (_p(0.5, 2, 25, 2, 5, 1.2), [LARGE]),              # window not a multiple of 3
    "win33": (_p(0.5, 0, 33, 5, 5, 1.2), [SMALL, LARGE]),       # single level; halo 16; 264 px = two 224-column bands; five iterations
    "win63": (_p(0.5, 1, 63, 2, 5, 1.1), [SMALL]),              # window wider than half the frame: clamped rows and columns dominate
    "win3": (_p(0.5, 2, 3, 3, 5, 1.2), [SMALL]),                # smallest window (ungated: the float32 oracle is 4.9e-3 from the float64 one)
    "scale08": (_p(0.8, 4, 15, 3, 5, 1.2), [SMALL, LARGE]),     # five levels of non-dyadic sizes, upsampling x 1.25
    "iter1": (_p(0.5, 3, 15, 1, 5, 1.2), [SMALL]),              # one iteration per level on the fused kernel: the pyramid step and the magnitude range in ONE launch
    "deep4": (_p(0.5, 4, 15, 3, 5, 1.2), [(512, 520)]),         # scale 1/16, 39-tap smoothing (5 sigma = 37.5 -> 38 | 1)
    "deep5": (_p(0.5, 5, 15, 3, 5, 1.2), [(1024, 1056)]),       # scale 1/32, 79 taps: the limit
}
SINGLE_PAIR = ("deep4", "deep5")     # one pair per call (frame size)
UNGATED = ("win3",)                  # not well posed by design: finite, bit-stable, paths equal - no parity gate
# Gated on the mean term only: the two oracles disagree at isolated pixels.  deep5 by design (outliers of 2e-2); deep4 is the one case that
# failed the well-posedness rule when it was measured (max |fp32 - fp64| 2.6e-3 at 512 x 520 on the smooth pair, mean 2.1e-6) and was moved
# here instead of being dropped.  tests/test_flow_params_cpu.py holds what "isolated" means.
MEAN_ONLY = ("deep4", "deep5")
OUTLIER_SHARE = 1e-3                 # MEAN_ONLY: at most this share of the flow components is further than WELL_POSED from the float64 oracle
WELL_POSED = 1e-3                    # max |oracle fp32 - oracle fp64|: tests/test_gpu_flow_content.py's rule

SMOOTH = ("smooth", fc.SHIFTS[0], 3)     # the content the issue's figures were measured on
SECOND = ("noise", fc.SHIFTS[0], 6)      # a second kind: the noisy texture under the same shift (tests/flow_cases.py lists it at 97 x 131)
THIRD = ("smooth", fc.ROTZOOMS[0], 1)    # fills the batch of three: bits only, never gated


def pair_case(size, content):
    kind, motion, seed = content
    return (size[0], size[1], kind, motion, seed)


def set_sizes():
    return [(name, size) for name, (_, sizes) in SETS.items() for size in sizes]


def batch_of(name, size):
    """The pairs of one GPU call for a set at a size: three different contents, or the smooth pair alone for the large frames."""
    if name in SINGLE_PAIR:
        return [pair_case(size, SMOOTH)]
    return [pair_case(size, SMOOTH), pair_case(size, SECOND), pair_case(size, THIRD)]


def gated_cases():
    """(set, pair case) of every parity-gated case: the smooth pair of every set at every size, and the second kind at the set's first
    size (not for the two large single-pair sets: their oracles take seconds)."""
    out = []
    for name, (_, sizes) in SETS.items():
        if name in UNGATED:
            continue
        for size in sizes:
            out.append((name, pair_case(size, SMOOTH)))
        if name not in SINGLE_PAIR:
            out.append((name, pair_case(sizes[0], SECOND)))
    return out


def gated_id(item):
    return f"{item[0]}-{fc.case_id(item[1])}"


@functools.lru_cache(maxsize=None)
def _reference(items, case):
    a, b = fc.make_pair(case)
    ga, gb = flow_ref.bgr2gray(a), flow_ref.bgr2gray(b)
    params = dict(items)
    f64, f32 = flow_ref.farneback(ga, gb, dtype=np.float64, **params), flow_ref.farneback(ga, gb, **params)
    f64.setflags(write=False)
    f32.setflags(write=False)
    return f64, f32


def reference(params, case):
    """-> (the oracle's flow in float64, in float32) of the pair under the six parameters, computed once; do not write into them."""
    return _reference(tuple(sorted(params.items())), case)


def oracle_plan(H, W, pyr_scale, levels):
    """[(h, w, ksize, sigma)] coarsest first, as oracle/flow_ref.farneback derives them (scale = pyr_scale ** k)."""
    used = flow_ref.pyramid_levels(H, W, pyr_scale, levels)
    out = []
    for k in range(used, -1, -1):
        scale = pyr_scale ** k
        sigma = (1.0 / scale - 1) * 0.5
        out.append((flow_ref.cv_round(H * scale), flow_ref.cv_round(W * scale), max(flow_ref.cv_round(sigma * 5) | 1, 3), sigma))
    return out


def parity_terms(got, ref64, ref32):
    """(mean ratio, max ratio) of tests/flow_cases.parity_ratio, separately."""
    e = np.abs(np.asarray(got, dtype=np.float64) - ref64)
    c = np.abs(ref32.astype(np.float64) - ref64)
    return float(e.mean() / c.mean()), float(e.max() / c.max())


def case_ratio(name, got, ref64, ref32):
    """The figure the gate applies to: flow_cases.parity_ratio, or its mean term alone for the sets of MEAN_ONLY."""
    return parity_terms(got, ref64, ref32)[0] if name in MEAN_ONLY else fc.parity_ratio(got, ref64, ref32)


def parity_gate():
    """tests/flow_cases.parity_gate's rule on a JSON of its own: the next power of two above the worst ratio recorded in
    profiles/flow_params_parity.json (tools/flow_params_parity.py measures it on the GPU), capped at flow_cases.PARITY_CAP."""
    with open(PARITY_JSON) as f:
        ratio = float(json.load(f)["flow_vs_oracle_fp32"]["worst_ratio"])
    gate = 1.0
    while gate <= ratio:
        gate *= 2.0
    return min(gate, fc.PARITY_CAP)
