"""ResNet-50 on every canvas size, the host half (csrc/host_logic.cpp: rn_canvas_geometry with flags, rn_plan on a flagged canvas, rn_stem_plan):
under RELAX_RN_CANVAS_ANY every Hc, Wc in [64, 1024] is a canvas, the maps follow torch's floor rule and may be odd; with flags 0 everything is
what it was.  The host library is built as tests/test_resnet_canvas_cpu.py builds it.  No GPU."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import pytest

from tests import rn_schedule_checks as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANY = 1                                                       # RELAX_RN_CANVAS_ANY
TAP_CHANNELS = (64, 256, 256, 256, 512, 512, 512, 512, 1024, 1024, 1024, 1024, 2048, 2048, 2048)
CANVASES = ((65, 67), (70, 100), (95, 98), (230, 232), (270, 480), (540, 960), (1023, 65))
SIZE_NAMES = ("x0", "big", "t1", "t2", "gap_ws", "block_max", "floats_f32", "floats_x6")
STEM_224, STEM_TILES, STEM_ANY = range(3)
POOL_EVEN, POOL_ANY = range(2)
PLAN_INTS = 4 + 16 * len(rc.FIELDS)


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("host_anysize") / "libhost.so"
    src = os.path.join(ROOT, "relax-vqa_amd", "csrc", "host_logic.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-DRELAX_HOST_TEST_API", src, "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    for name in ("relax_host_rn_plan_canvas", "relax_host_rn_canvas_geometry", "relax_host_rn_canvas_geometry_ex", "relax_host_rn_plan_canvas_ex",
                 "relax_host_rn_stem_plan_ex"):
        getattr(lib, name).restype = C.c_int
    return lib


def geometry_ex(lib, Hc, Wc, flags):
    """([(h, w)] * 15, sizes dict), or the message of a refused canvas (and then nothing was written)."""
    taps = (C.c_int * 30)(*([-77] * 30))
    sizes = (C.c_int64 * 8)(*([-77] * 8))
    err = C.create_string_buffer(256)
    if lib.relax_host_rn_canvas_geometry_ex(Hc, Wc, flags, taps, sizes, err, 256) != 0:
        assert all(v == -77 for v in taps) and all(v == -77 for v in sizes), "a refused canvas must leave no geometry"
        return err.value.decode()
    return [(taps[2 * t], taps[2 * t + 1]) for t in range(15)], dict(zip(SIZE_NAMES, sizes))


def geometry_old(lib, Hc, Wc):
    taps = (C.c_int * 30)(*([-77] * 30))
    sizes = (C.c_int64 * 8)(*([-77] * 8))
    err = C.create_string_buffer(256)
    if lib.relax_host_rn_canvas_geometry(Hc, Wc, taps, sizes, err, 256) != 0:
        return err.value.decode()
    return [(taps[2 * t], taps[2 * t + 1]) for t in range(15)], dict(zip(SIZE_NAMES, sizes))


def plan_ex(lib, opts, req, Hc, Wc, flags, max_slots=rc.IMG_SLOTS):
    out = (C.c_int * PLAN_INTS)(*([-77] * PLAN_INTS))
    err = C.create_string_buffer(256)
    if lib.relax_host_rn_plan_canvas_ex((C.c_int * 6)(*opts), (C.c_int * 5)(*req), Hc, Wc, flags, max_slots, out, err, 256) != 0:
        assert all(v == -77 for v in out), "a refused plan must leave no plan"
        return err.value.decode()
    return list(out)


def stem_plan(lib, Hc, Wc, flags):
    out = (C.c_int * 3)(-77, -77, -77)
    err = C.create_string_buffer(256)
    if lib.relax_host_rn_stem_plan_ex(Hc, Wc, flags, out, err, 256) != 0:
        assert list(out) == [-77] * 3
        return err.value.decode()
    return dict(zip(("stem_form", "pool_form", "stem_fused_mean"), out))


def floor_maps(Hc, Wc):
    """torch's floor((n + 2 p - k) / s) + 1, stage by stage, written out: the 15 taps' (h, w)"""
    def side(n):
        n0 = (n + 2 * 3 - 7) // 2 + 1                        # conv1 7x7 / 2 pad 3
        n1 = (n0 + 2 * 1 - 3) // 2 + 1                       # max-pool 3x3 / 2 pad 1
        out, n = [n0], n1
        for blocks, taps, stride in ((3, 3, 1), (4, 4, 2), (6, 4, 2), (3, 3, 2)):
            for i in range(blocks):
                n = (n + 2 - 3) // (stride if i == 0 else 1) + 1
                if i < taps:
                    out.append(n)
        return out
    return list(zip(side(Hc), side(Wc)))


def wanted_sizes(Hc, Wc, taps):
    """what the forward's tensors need, from the maps alone"""
    hw0, hw1 = taps[0][0] * taps[0][1], taps[1][0] * taps[1][1]
    groups = [h * w // (16 if h * w % 16 == 0 else 4) * c for (h, w), c in zip(taps, TAP_CHANNELS) if h * w % 4 == 0]
    return dict(x0=Hc * Wc * 4, big=max(hw0 * 64, hw1 * 256), t1=hw1 * 128, t2=hw1 * 64, gap_ws=max([16 * 2048] + groups),
                block_max=-(-hw1 * 16 // 256))


# ---- geometry ------------------------------------------------------------------------------------------------------------------------------
def test_every_size_follows_the_floor_rule_and_multiples_of_32_keep_their_ints(host_lib):
    for v in range(64, 1025):
        for Hc, Wc in ((v, 64), (64, v)):
            got = geometry_ex(host_lib, Hc, Wc, ANY)
            assert not isinstance(got, str), got
            taps, sizes = got
            assert taps == floor_maps(Hc, Wc), (Hc, Wc)
            want = wanted_sizes(Hc, Wc, taps)
            for k in ("x0", "t1", "t2", "gap_ws"):
                assert sizes[k] == want[k], (Hc, Wc, k)
            # never smaller than what the maps need: the stem's output AND a layer1 block's output live in `big`; one word per 256-thread block
            # (the other side is 64 here, so these blocks are whole: test_block_max_rounds_up_where_the_blocks_are_ragged has a ragged case)
            assert sizes["big"] >= want["big"] and sizes["block_max"] >= want["block_max"] and sizes["block_max"] % 64 == 0, (Hc, Wc)
            assert all(s % 4 == 0 for s in sizes.values()), (Hc, Wc)               # every carving stays 16-byte aligned
            assert sizes["floats_f32"] == sizes["x0"] + 3 * sizes["big"] + sizes["t1"] + sizes["t2"] + sizes["gap_ws"] + 2048
            assert sizes["floats_x6"] == (sizes["x0"] + 3 * sizes["big"] + 2 * (sizes["big"] * 3 // 2) + (sizes["t1"] + sizes["t2"]) * 3 // 2
                                          + sizes["gap_ws"] + 2048 + 3 * 64 + sizes["block_max"])
            old = geometry_old(host_lib, Hc, Wc)
            if v % 32 == 0:
                assert old == (taps, sizes), (Hc, Wc)                              # int for int, the eight sizes included
                assert geometry_ex(host_lib, Hc, Wc, 0) == old
            else:
                assert isinstance(old, str) and geometry_ex(host_lib, Hc, Wc, 0) == old


def test_the_issues_table_of_maps(host_lib):
    table = {(65, 67): [(33, 34), (17, 17), (9, 9), (5, 5), (3, 3)], (70, 100): [(35, 50), (18, 25), (9, 13), (5, 7), (3, 4)],
             (95, 98): [(48, 49), (24, 25), (12, 13), (6, 7), (3, 4)], (230, 232): [(115, 116), (58, 58), (29, 29), (15, 15), (8, 8)],
             (270, 480): [(135, 240), (68, 120), (34, 60), (17, 30), (9, 15)]}
    for (Hc, Wc), maps in table.items():
        taps, _ = geometry_ex(host_lib, Hc, Wc, ANY)
        assert [taps[0], taps[1], taps[4], taps[8], taps[12]] == maps, (Hc, Wc)
        assert taps[1:4] == [maps[1]] * 3 and taps[4:8] == [maps[2]] * 4 and taps[8:12] == [maps[3]] * 4 and taps[12:] == [maps[4]] * 3


def test_block_max_rounds_up_where_the_blocks_are_ragged(host_lib):
    """1023 x 1023: layer1 is 256 x 256 - whole blocks; 1000 x 1016: 250 x 254 x 16 = 1 016 000 threads = 3968.75 blocks: 3969 words, and the
    round-down of before, 3968, is exactly the multiple of 64 below it"""
    taps, sizes = geometry_ex(host_lib, 1000, 1016, ANY)
    need = taps[1][0] * taps[1][1] * 16
    assert taps[1] == (250, 254) and need % 256 != 0 and need // 256 == 3968 == 62 * 64
    assert sizes["block_max"] >= -(-need // 256) and sizes["block_max"] == 4032
    # 65 x 67: the layer1 output (17 x 17 x 256) is larger than the stem's (33 x 34 x 64)
    taps, sizes = geometry_ex(host_lib, 65, 67, ANY)
    assert 17 * 17 * 256 > 33 * 34 * 64 and sizes["big"] == 17 * 17 * 256


@pytest.mark.parametrize("bad", (63, 1025, 0, -64))
def test_refusals_under_the_flag_name_the_value_and_the_canvas(host_lib, bad):
    for Hc, Wc, axis in ((bad, 100, "height"), (100, bad, "width"), (bad, bad, "height")):
        msg = geometry_ex(host_lib, Hc, Wc, ANY)
        assert isinstance(msg, str) and f"canvas {axis} {bad} is not in [64, 1024] (canvas {Hc} x {Wc})" in msg, msg
        assert plan_ex(host_lib, (3, 1, 1, 1, 1, 1), rc.REQUESTS["clip"], Hc, Wc, ANY) == msg
        assert stem_plan(host_lib, Hc, Wc, ANY) == msg


@pytest.mark.parametrize("flags", (2, 3, 4, 0x100, -2))
def test_an_unknown_flag_bit_is_refused_by_name(host_lib, flags):
    msg = geometry_ex(host_lib, 96, 160, flags)
    assert isinstance(msg, str) and f"canvas flags {flags} have unknown bits {flags & ~1}" in msg and "RELAX_RN_CANVAS_ANY" in msg, msg
    assert "(canvas 96 x 160)" in msg
    assert plan_ex(host_lib, (3, 1, 1, 1, 1, 1), rc.REQUESTS["clip"], 96, 160, flags) == msg


def test_flags_0_refuses_100_with_todays_message(host_lib):
    want = "resnet50: canvas width 100 is not a multiple of 32 in [64, 1024] (canvas 64 x 100)"
    assert geometry_ex(host_lib, 64, 100, 0) == want == geometry_old(host_lib, 64, 100)
    assert plan_ex(host_lib, (3, 1, 1, 1, 1, 1), rc.REQUESTS["clip"], 64, 100, 0) == want
    for h in (230, 232, 270):
        assert f"canvas height {h} is not a multiple of 32 in [64, 1024]" in geometry_ex(host_lib, h, 224, 0)


# ---- plans ---------------------------------------------------------------------------------------------------------------------------------
def all_options():
    for precision in (2, 3):
        for flags in itertools.product((0, 1), repeat=5):
            yield (precision,) + flags


class _Map:
    """stands where rn_schedule_checks keeps the side of a square map: its `** 2` is the map's pixel count"""
    def __init__(self, h, w):
        self.hw = h * w

    def __pow__(self, e):
        assert e == 2
        return self.hw


def _block_maps(taps):
    """the output map of each of the 16 blocks (layer3's untapped blocks 4, 5 have layer3's map)"""
    return [taps[1]] * 3 + [taps[4]] * 4 + [taps[8]] * 6 + [taps[12]] * 3


def _split(o):
    stem = dict(zip(("conv1_h2", "pool_f32", "s_stem", "n_slots"), o[:4]))
    return stem, [rc.Block(o[4 + i * len(rc.FIELDS):4 + (i + 1) * len(rc.FIELDS)]) for i in range(16)]


def _check_forms(stem, blocks, stemp, taps, where):
    """every fused form only on maps its rn_maps_* predicate (restated) takes; the slot budget"""
    assert 0 <= stem["n_slots"] <= rc.IMG_SLOTS, where
    owned = [stem["s_stem"]] + [getattr(q, f) for q in blocks for f in ("s_c1", "s_t1", "s_t1m", "s_t2", "s_out", "s_dr_out")]
    assert sorted(s for s in owned if s >= 0) == list(range(stem["n_slots"])), where
    h1, w1 = taps[1]
    if stem["s_stem"] >= 0 and stemp["pool_form"] == POOL_EVEN:                  # rn_maps_pool_maxima: whole blocks per image
        assert (h1 * w1 * 16) % 256 == 0, where
    if stemp["pool_form"] == POOL_EVEN:
        assert taps[0][0] % 2 == 0 and taps[0][1] % 2 == 0, where
    if stemp["stem_form"] != STEM_ANY:                                           # whole 16 x 16 tiles of an even canvas
        assert taps[0][0] % 16 == 0 and taps[0][1] % 16 == 0, where
    if stemp["stem_fused_mean"]:                                                 # rn_maps_stem_fused_mean: a 16-pixel group never crosses a row end
        assert taps[0][1] % 16 == 0 and (taps[0][0] * taps[0][1]) % 16 == 0, where
    prev_form, prev_sample = (rc.F32 if stem["pool_f32"] else rc.SP3), rc.NO_SAMPLE
    h, w = h1, w1
    for b, (q, (ho, wo)) in enumerate(zip(blocks, _block_maps(taps))):
        stride, has_down = rc.GEOM[b][3], rc.GEOM[b][4]
        assert (ho, wo) == ((h - 1) // stride + 1, (w - 1) // stride + 1), (where, b)
        at = (where, b, (ho, wo))
        assert (q.in_form, q.in_sample) == (prev_form, prev_sample), at
        if q.form in (rc.B2B, rc.B2BX2, rc.B2BDOWN):                             # rn_maps_b2b
            assert ho * wo >= 256 and (ho * wo) % 16 == 0 and q.in_form == rc.F32, at
        assert (q.form == rc.B2BDOWN) == (q.in_sample == rc.SAMPLE_H2), at
        if q.in_sample == rc.SAMPLE_SP3:
            assert q.form in (rc.X6, rc.EARLY) and has_down, at
        if q.fuse_mean:                                                          # rn_maps_fused_mean
            assert (ho * wo) % 4 == 0, at
        if q.form == rc.H2FORM and q.fuse_mean:
            assert (ho * wo) % 16 != 0, at
        if q.out_sample != rc.NO_SAMPLE:                                         # rn_maps_sample2
            assert ho % 2 == 0 and wo % 2 == 0 and q.form in (rc.B2B, rc.B2BX2, rc.B2BDOWN), at
        if q.want_mean and not q.fuse_mean:
            assert q.need32, at
        assert q.rows32 % (ho * wo) == 0, at
        prev_form, prev_sample = q.out_form, q.out_sample
        h, w = ho, wo
    assert (h, w) == taps[14]


@pytest.mark.parametrize("canvas", CANVASES, ids=lambda c: "%dx%d" % c)
def test_plans_under_the_flag(host_lib, canvas, monkeypatch):
    Hc, Wc = canvas
    taps, _ = geometry_ex(host_lib, Hc, Wc, ANY)
    maps = _block_maps(taps)
    monkeypatch.setattr(rc, "SIDE", [_Map(h, w) for h, w in maps])               # rn_schedule_checks' dataflow checks, on this canvas' maps
    stemp = stem_plan(host_lib, Hc, Wc, ANY)
    assert stemp["stem_form"] == STEM_ANY and stemp["pool_form"] == POOL_ANY
    assert stemp["stem_fused_mean"] == int(taps[0][1] % 16 == 0)
    # the one statement of check_case that is about 224 only: "a tapped map of whole 4-row groups fuses its mean".  The f16x2 blocks fuse it on
    # 4-row groups only where the map is NOT whole 16-row groups (as at 448 x 448 today); on such a canvas check_case runs on the requests
    # without a layer stack, and the forms and the dataflow of the others are checked by _check_forms
    whole16 = any(h * w % 16 == 0 for h, w in maps[7:])
    cases = 0
    for opts in all_options():
        fixed = None
        for name, req in rc.REQUESTS.items():
            where = (canvas, opts, name)
            o = plan_ex(host_lib, opts, req, Hc, Wc, ANY)
            assert isinstance(o, list), o
            stem, blocks = _split(o)
            _check_forms(stem, blocks, stemp, taps, where)
            h2_blocks = any(q.form == rc.H2FORM for q in blocks)
            if not (whole16 and h2_blocks and req[1] > 0):
                rc.check_case(stem, blocks, req, where)
                cases += 1
            forms = [q.form for q in blocks]
            fixed = fixed or forms
            assert forms == fixed                                                # the forms do not look at the request
            msg = plan_ex(host_lib, opts, req, Hc, Wc, ANY, stem["n_slots"] - 1)
            assert isinstance(msg, str) and "%d per-image scale slots used" % stem["n_slots"] in msg
            if opts == (3, 1, 1, 1, 1, 1):
                # the any-map max-pool posts its maxima on every map: layer1 / layer2 keep the f16x2 3x3
                assert stem["s_stem"] >= 0 and stem["conv1_h2"] == 1
                assert all(q.form != rc.X6 for q in blocks[:7]), (where, forms)
                assert all(q.form == rc.H2FORM for q in blocks[7:]), where
    assert cases >= 32 * 2


def test_an_old_canvas_under_the_flag_is_the_old_plan_and_the_old_forms(host_lib):
    for Hc, Wc in ((96, 160), (224, 224), (288, 512), (64, 64), (1024, 64)):
        want_stem = dict(stem_form=STEM_224 if (Hc, Wc) == (224, 224) else STEM_TILES, pool_form=POOL_EVEN, stem_fused_mean=1)
        assert stem_plan(host_lib, Hc, Wc, ANY) == want_stem == stem_plan(host_lib, Hc, Wc, 0)
        for opts in all_options():
            for req in rc.REQUESTS.values():
                out = (C.c_int * PLAN_INTS)()
                err = C.create_string_buffer(256)
                assert host_lib.relax_host_rn_plan_canvas((C.c_int * 6)(*opts), (C.c_int * 5)(*req), Hc, Wc, rc.IMG_SLOTS, out, err, 256) == 0
                assert plan_ex(host_lib, opts, req, Hc, Wc, ANY) == list(out) == plan_ex(host_lib, opts, req, Hc, Wc, 0)


def test_the_plan_struct_keeps_its_size_and_the_96x160_plan_its_ints(host_lib):
    """relax_host_rn_plan_canvas copies sizeof(RnPlan) bytes out: exactly 4 + 16 * 23 ints are written, the guard ints behind them stay"""
    assert PLAN_INTS == 4 + 16 * 23
    n = PLAN_INTS + 8
    out = (C.c_int * n)(*([-77] * n))
    err = C.create_string_buffer(256)
    opts, req = (3, 1, 1, 1, 1, 1), rc.REQUESTS["layer stack + pool"]
    assert host_lib.relax_host_rn_plan_canvas((C.c_int * 6)(*opts), (C.c_int * 5)(*req), 96, 160, rc.IMG_SLOTS, out, err, 256) == 0
    o = list(out)
    assert o[PLAN_INTS:] == [-77] * 8 and o[PLAN_INTS - 1] != -77
    stem, blocks = _split(o[:PLAN_INTS])
    # the plan of tests/test_resnet_canvas_cpu.py's 96 x 160 case, written out
    assert stem == dict(conv1_h2=1, pool_f32=1, s_stem=0, n_slots=stem["n_slots"]) and 0 < stem["n_slots"] <= rc.IMG_SLOTS
    assert [q.form for q in blocks] == [rc.B2BX2, rc.B2B, rc.B2B] + [rc.EARLY] * 4 + [rc.H2FORM] * 9
    assert not any(q.fuse_mean for q in blocks[13:]) and all(q.need32 for q in blocks[13:])
    assert [q.rows32 for q in blocks[:3]] == [rc.N_IMG * 24 * 40] * 3


# ---- sanitizers ----------------------------------------------------------------------------------------------------------------------------
def test_the_any_size_host_logic_runs_clean_under_asan_and_ubsan(tmp_path):
    """tests/rn_anysize_san_main.cpp + csrc/host_logic.cpp under AddressSanitizer + UBSan, built as tests/test_conv_hoelder_cpu.py builds its
    program: a plain child process with its own main, nothing preloaded, nothing loaded into Python."""
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    san = ["-fsanitize=address,undefined"]
    probe = ["-x", "c++", "-", "-o", os.devnull]
    if subprocess.run([cxx, *san, *probe], input="int main(){}", capture_output=True, text=True).returncode != 0:
        pytest.skip(f"{cxx} -fsanitize=address,undefined cannot link on this machine")
    static = ["-static-libasan", "-static-libubsan"]
    if subprocess.run([cxx, *san, *static, *probe], input="int main(){}", capture_output=True, text=True).returncode == 0:
        san += static
    csrc = os.path.join(ROOT, "relax-vqa_amd", "csrc")
    exe = str(tmp_path / "rn_anysize_san")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-I", csrc, *san, "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    os.path.join(ROOT, "tests", "rn_anysize_san_main.cpp"), os.path.join(csrc, "host_logic.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "rn_anysize_san: OK" in res.stdout
    assert "ERROR" not in res.stderr and "runtime error" not in res.stderr, res.stderr
