"""host::vgg_plan (csrc/host_logic.cpp) through its test export: the call, the grid of options and requests, and the checks of one plan
(helper of tests/test_vgg16_plan_cpu.py and tests/test_gpu_vgg16_plan.py; pure Python)."""
import ctypes as C
import itertools

FIELDS = "route layer side cin cout in_ out32 out_planes want_mean gap_group want_export no_split s_in s_out s_in_max measure_max".split()
CONV11, CONV_H3, CONV_X6H2, CONV_X6, CONV_F32, POOL_H2, POOL_SP3, POOL_F32 = range(8)      # VggRoute
NONE, A32, PLANES0, PLANES1, FC1, FC2 = range(6)                                           # VggBuffer
ARENA = ("a32", "planes0", "planes1", "groups", "fc1", "fc2", "slots", "floats")           # in carving order; `floats` is the total
STEPS, SLOTS, CHUNK = 20, 24, 32
FLOATS_PER_IMAGE = 13054024            # 3 211 264 + 2 x 4 816 896 + 200 704 + 2 x 4096 + 3 x 24
POOLS = (POOL_H2, POOL_SP3, POOL_F32)
# read kinds of relax_profile_read a contraction launch of a route is counted in (tests/gpu_common.py: ROUTE_KINDS); every f16x2 launch of
# VGG-16 is of the convolution form, so none is a plain f16x2 GEMM (kind 9)
ROUTE_KIND = {CONV_H3: 7, CONV_X6H2: 7, CONV_X6: 3, CONV_F32: 0}

TAP_MASKS = {"none": 0, "all 15": 0x7FFF, "tap 0": 1 << 0, "tap in front of a pool": 1 << 3, "fc1": 1 << 13, "fc2": 1 << 14}
WANTS = {"layer stack only": (1, 0), "pool only": (0, 1), "both": (1, 1), "neither": (0, 0)}    # want_layer_stack, want_pool


def requests():
    """name -> (N, want_layer_stack, want_pool, taps); `neither` goes with taps only"""
    out = {}
    for (wname, (ls, pool)), (tname, taps), n in itertools.product(WANTS.items(), TAP_MASKS.items(), (1, CHUNK)):
        if wname == "neither" and taps == 0:
            continue
        out[f"{wname}, taps {tname}, N={n}"] = (n, ls, pool, taps)
    return out


class Row:
    def __init__(self, ints):
        self.__dict__.update(zip(FIELDS, ints))


def _call(lib, precision, req, max_slots):
    """relax_host_vgg_plan -> (ints, arena values), or the message when the plan is refused (and then nothing was written)"""
    lib.relax_host_vgg_plan.restype = C.c_int
    n = 3 + STEPS * len(FIELDS) + 26
    out = (C.c_int * n)(*([-77] * n))
    arena = (C.c_int64 * (len(ARENA) + 1))(*([-77] * (len(ARENA) + 1)))
    err = C.create_string_buffer(256)
    rc = lib.relax_host_vgg_plan((C.c_int * 1)(precision), (C.c_int * 4)(*req), max_slots, out, arena, err, 256)
    if rc != 0:
        assert rc == -1 and all(v == -77 for v in out) and all(v == -77 for v in arena), "a refused plan must leave no plan"
        return err.value.decode()
    return list(out), list(arena)


def plan(lib, precision, req, max_slots=SLOTS):
    """(head dict, [Row] * n_rows, arena dict), or the message when the plan is refused"""
    res = _call(lib, precision, req, max_slots)
    if isinstance(res, str):
        return res
    o, arena = res
    head = dict(zip(("n_slots", "classifier", "n_rows"), o[:3]))
    rows = [Row(o[3 + i * len(FIELDS):3 + (i + 1) * len(FIELDS)]) for i in range(STEPS)]
    return head, rows[:head["n_rows"]], dict(zip(ARENA, arena))


def geometry(lib):
    """[(side, pool behind it)] of the 13 convolutions: the tail of the plan's integers"""
    g = _call(lib, 3, (1, 1, 1, 0), SLOTS)[0][3 + STEPS * len(FIELDS):]
    return [(g[2 * i], g[2 * i + 1]) for i in range(13)]


def arena_bytes(lib, n):
    """vgg_arena_bytes(n): the workspace of a call on n images (the value behind the plan's arena offsets)"""
    return _call(lib, 3, (n, 1, 1, 0), SLOTS)[1][len(ARENA)]


def buffer_floats(arena):
    """floats per image of every VggBuffer: up to the next part of the arena"""
    size = {name: arena[nxt] - arena[name] for name, nxt in zip(ARENA[:-1], ARENA[1:])}
    return {A32: size["a32"], PLANES0: size["planes0"], PLANES1: size["planes1"], FC1: size["fc1"], FC2: size["fc2"]}, size["groups"]


def check_case(precision, head, rows, arena, req, where):
    """Slots, slot order, dataflow, fp32 copies, group sums and sizes of one plan"""
    N, want_ls, want_pool, taps = req
    h2, x6 = precision == 3, precision >= 2
    # ---- slots: every slot below n_slots belongs to one step (the classifier's two are counted whether or not it runs)
    assert head["n_slots"] == (20 if h2 else 0), where
    classifier = int(bool(want_pool or taps >> 13 & 3))
    assert head["classifier"] == classifier and head["n_rows"] == (STEPS if classifier else STEPS - 2), where
    owned = [q.s_out for q in rows if q.s_out >= 0]
    assert owned == list(range(len(owned))) and len(owned) == (len(rows) if h2 else 0) and head["n_slots"] in (0, STEPS), where
    # ---- the steps: 13 convolutions with a pool behind five of them, then fc1 and fc2; without the classifier the forward ends behind pool5
    assert [q.layer for q in rows if q.route not in POOLS] == list(range(15 if classifier else 13)), where
    assert rows[0].route == CONV11 and rows[17].route in POOLS and rows[17].layer == 12, where
    # ---- arena: today's carving order, its total, and every tensor inside its buffer
    assert [arena[k] for k in ARENA] == sorted(arena[k] for k in ARENA) and arena["a32"] == 0 and arena["floats"] == FLOATS_PER_IMAGE, where
    assert arena["floats"] - arena["slots"] == 3 * SLOTS, where
    cap, cap_groups = buffer_floats(arena)
    have_max, have_scale = set(), set()
    holds = None                 # (buffer, form) the previous producing step left for the next one: form "planes" or "rows"
    copies = {}                  # buffer -> the step whose fp32 copy lies there, until something overwrites it
    for r, q in enumerate(rows):
        w = (where, r)
        pooling, fc = q.route in POOLS, q.layer >= 13
        out_side = q.side // 2 if pooling else q.side
        out_floats = out_side * out_side * q.cout
        # ---- slot order: a scale from a maximum an earlier step measured; the input's scale written before this step
        if h2:
            assert q.s_out >= 0 and (q.s_in >= 0) == (r > 0 and not pooling) and (q.s_in_max >= 0) == (r > 0), w
            assert q.s_in < 0 or q.s_in in have_scale, w
            assert q.s_in_max < 0 or q.s_in_max in have_max, w
            have_scale.add(q.s_out)              # conv1_1: the kernel writes its static scale itself
            if q.measure_max:
                have_max.add(q.s_out)
            if pooling:                           # a new scale slot; the maximum stays the producer's
                assert q.s_in_max == rows[r - 1].s_out, w
                assert r + 1 == len(rows) or (rows[r + 1].s_in_max, rows[r + 1].s_in) == (q.s_in_max, q.s_out), w
            assert q.measure_max == int(not pooling and (not fc or q.out_planes != NONE)), w
        else:
            assert (q.s_in, q.s_out, q.s_in_max, q.measure_max) == (-1, -1, -1, 0), w
        # ---- dataflow: the step reads what the previous producing step wrote, and writes no buffer its own input sits in
        if r == 0:
            assert q.in_ == NONE, w
        elif pooling:
            assert q.in_ == rows[r - 1].out32 != NONE and copies[q.in_] == r - 1, w      # the fp32 map of the convolution in front
        else:
            assert holds is not None and q.in_ == holds[0] and holds[1] == ("planes" if x6 else "rows"), w
        written = [b for b in (q.out32, q.out_planes) if b != NONE]
        assert written and q.in_ not in written and len(set(written)) == len(written), w
        for b in written:
            assert out_floats * (1.5 if (b == q.out_planes and precision == 2) else 1) <= cap[b], w     # split planes: 6 B a value
            copies.pop(b, None)
        if q.out32 != NONE:
            copies[q.out32] = r
        if x6:
            # planes for the next contraction: not from a convolution a pool follows (the pool writes them), not from fc2
            pool_behind = r + 1 < len(rows) and rows[r + 1].route in POOLS
            assert (q.out_planes != NONE) == (not pool_behind and q.layer != 14 or pooling), w
            if q.out_planes != NONE:
                holds = (q.out_planes, "planes")
        else:
            assert q.out_planes == NONE and q.out32 != NONE, w
            holds = (q.out32, "rows")
        # ---- the fp32 copy exists exactly where a pool, an export, a launch_gap mean or the pool vector reads it (fp32 rows: it is the tensor)
        if not pooling:
            tapped = bool(taps >> q.layer & 1)
            assert q.want_export == int(tapped) and q.want_mean == int(bool(want_ls) and not fc), w
            pool_next = r + 1 < len(rows) and rows[r + 1].route in POOLS
            mean_reads = q.want_mean and q.gap_group == 0
            if x6:
                assert (q.out32 != NONE) == bool(pool_next or tapped or mean_reads or q.layer == 14), w
                assert q.out32 == {13: FC1, 14: FC2}.get(q.layer, A32) or q.out32 == NONE, w
            # ---- fused mean: under planes every tap's, conv1_1's under every arithmetic; the group sums fit their part of the arena
            assert (q.gap_group > 0) == bool(q.want_mean and (x6 or r == 0)), w
            if q.gap_group:
                hw = q.side * q.side
                assert q.gap_group == (4 if q.route == CONV_H3 else 16 if hw % 16 == 0 else 4) and hw % q.gap_group == 0, w
                assert hw // q.gap_group * q.cout <= cap_groups, w
        else:
            assert (q.want_export, q.want_mean, q.gap_group) == (0, 0, 0) and q.cin == q.cout and q.side % 2 == 0, w
    if classifier:
        assert rows[-1].out32 == FC2 and rows[-1].out_planes == NONE, where        # what the pool vector and tap 14 read


def shape(rows):
    """what must not depend on the request: routes, geometry, no_split, buffers of the planes, slots"""
    return [(q.route, q.layer, q.side, q.cin, q.cout, q.in_, q.out_planes, q.no_split, q.s_in, q.s_out, q.s_in_max, q.measure_max) for q in rows]


def expected_routes(precision):
    """conv1_2 .. conv5_3, fc1, fc2"""
    if precision == 3:
        return [CONV_X6H2] * 3 + [CONV_H3] * 11
    return [CONV_X6 if precision == 2 else CONV_F32] * 14


def check_all(lib):
    cases = 0
    for precision in (0, 1, 2, 3):
        fixed = None
        for name, req in requests().items():
            where = (precision, name)
            head, rows, arena = plan(lib, precision, req)
            check_case(precision, head, rows, arena, req, where)
            routes = [q.route for q in rows if q.route not in POOLS]
            assert routes[0] == CONV11 and routes[1:] == expected_routes(precision)[:len(routes) - 1], where
            assert [q.route for q in rows if q.route in POOLS] == [{3: POOL_H2, 2: POOL_SP3}.get(precision, POOL_F32)] * 5, where
            assert all(q.no_split == int(q.route in (CONV_H3, CONV_X6H2, CONV_X6)) for q in rows), where
            full = plan(lib, precision, (req[0], 1, 1, 0))[1]
            fixed = fixed or shape(full)
            assert shape(rows) == fixed[:len(rows)], where
            n_slots = head["n_slots"]
            # one slot too few: refused with the message, no plan; exactly enough: accepted
            assert plan(lib, precision, req, n_slots - 1) == "vgg16: %d per-image scale slots used, %d reserved" % (n_slots, n_slots - 1), where
            assert not isinstance(plan(lib, precision, req, n_slots), str), where
            cases += 1
    return cases
