"""The ResNet-50 schedule (csrc/host_logic.cpp: rn_plan) checked over every option combination and request form, on the CPU.
`check_all(lib)` takes host_logic.cpp built with -DRELAX_HOST_TEST_API (tests/test_resnet_schedule_cpu.py: plain g++;
tests/host_logic_driver.py: under AddressSanitizer + UBSan) and returns the number of cases it ran."""
import ctypes as C
import itertools

FIELDS = ("form c1_h2 in_form in_sample out_form out_sample need32 rows32 want_mean fuse_mean want_export no_split handover pre_handover "
          "s_in_max s_in s_dr_in s_c1 s_t1 s_t1m s_t2 s_out s_dr_out").split()
X6, EARLY, B2B, B2BX2, B2BDOWN, H2FORM = range(6)
NONE, F32, SP3, H2 = range(4)
NO_SAMPLE, SAMPLE_SP3, SAMPLE_H2 = range(3)
IMG_SLOTS = 64          # kImgSlots of csrc/resnet50.hip: the per-image tables the arena reserves
N_IMG = 40
REQUESTS = {            # N, n_ls, pool_from, want_pool, exported taps
    "layer stack + pool": (N_IMG, N_IMG, 0, 1, 0),
    "pool only": (N_IMG, 0, 0, 1, 0),
    "layer stack only": (N_IMG, N_IMG, 0, 0, 0),
    "clip": (N_IMG, 15, 15, 1, 0),
    "all taps": (4, 4, 0, 1, 0x7FFF),
}
# torchvision's ResNet-50, restated: (cin, width, cout, stride, has_down, tap) and the side of each block's output map
GEOM, SIDE = [], []
_cin, _tap, _side = 64, 1, 56
for _st, (_blocks, _width, _taps) in enumerate(((3, 64, 3), (4, 128, 4), (6, 256, 4), (3, 512, 3))):
    for _i in range(_blocks):
        _stride = 2 if (_i == 0 and _st > 0) else 1
        _side //= _stride
        GEOM.append((_cin, _width, _width * 4, _stride, int(_i == 0), _tap if _i < _taps else -1))
        _tap += _i < _taps
        SIDE.append(_side)
        _cin = _width * 4


class Block:
    def __init__(self, ints):
        self.__dict__.update(zip(FIELDS, ints))


def plan(lib, opts, req, max_slots=IMG_SLOTS):
    """(stem dict, [Block] * 16), or the error message when the plan is refused (and then nothing was written)."""
    n = 4 + 16 * len(FIELDS)
    out = (C.c_int * n)(*([-77] * n))
    err = C.create_string_buffer(256)
    rc = lib.relax_host_rn_plan((C.c_int * 6)(*opts), (C.c_int * 5)(*req), max_slots, out, err, 256)
    if rc != 0:
        assert rc == -1 and all(v == -77 for v in out), "a refused plan must leave no plan"
        return err.value.decode()
    o = list(out)
    stem = dict(zip(("conv1_h2", "pool_f32", "s_stem", "n_slots"), o[:4]))
    return stem, [Block(o[4 + i * len(FIELDS):4 + (i + 1) * len(FIELDS)]) for i in range(16)]


def check_geometry(lib):
    g = (C.c_int * (16 * 9))()
    lib.relax_host_rn_geometry(g)
    rows = [tuple(g[i * 9:(i + 1) * 9]) for i in range(16)]
    assert [r[3:] for r in rows] == GEOM and [r[0] for r in rows] == list(range(16))
    assert [(r[1], r[2]) for r in rows] == [(l, i) for l, n in ((1, 3), (2, 4), (3, 6), (4, 3)) for i in range(n)]


def check_case(stem, blocks, req, where):
    N, n_ls, pool_from, want_pool, taps = req
    pool_from_stack = bool(want_pool and n_ls > 0 and pool_from == 0 and n_ls == N)
    # ---- slot budget: every slot below n_slots is handed out exactly once
    assert 0 <= stem["n_slots"] <= IMG_SLOTS, where
    owned = [stem["s_stem"]] + [getattr(q, f) for q in blocks for f in ("s_c1", "s_t1", "s_t1m", "s_t2", "s_out", "s_dr_out")]
    assert sorted(s for s in owned if s >= 0) == list(range(stem["n_slots"])), where
    have_max = {stem["s_stem"]} - {-1}        # slots whose maximum has been measured / whose scale has been computed, so far
    have_scale = set()

    def scale(slot, *maxima):
        assert slot >= 0 and all(m in have_max for m in maxima), (where, slot, maxima)
        have_scale.add(slot)

    prev_form, prev_sample, prev = (F32 if stem["pool_f32"] else SP3), NO_SAMPLE, None
    for b, q in enumerate(blocks):
        w = (where, b)
        cin, width, cout, stride, has_down, tap = GEOM[b]
        hwo, last = SIDE[b] ** 2, b == 15
        # ---- dataflow: the input is what the producer wrote
        assert (q.in_form, q.in_sample) == (prev_form, prev_sample), w
        if prev is not None:
            assert q.s_in_max == prev.s_out and q.s_dr_in == prev.s_dr_out, w
            assert q.s_in == (prev.s_out if prev.out_form == H2 else -1), w
        else:
            assert q.s_in_max == stem["s_stem"] and q.s_in == -1 and q.s_dr_in == -1, w
        b2b = q.form in (B2B, B2BX2, B2BDOWN)
        if q.in_sample != NO_SAMPLE:                       # the sample lies beside fp32 rows, and is read by this block's downsample branch only
            assert q.in_form == F32 and has_down, w
            assert (q.form == B2BDOWN) == (q.in_sample == SAMPLE_H2) and (q.form in (X6, EARLY)) == (q.in_sample == SAMPLE_SP3), w
        assert (q.form == B2BDOWN) <= (q.in_sample == SAMPLE_H2 and q.s_dr_in >= 0), w
        if q.form == H2FORM:
            assert q.in_form == H2 and q.s_in >= 0 and not q.c1_h2 and not q.handover, w
            assert b >= 7 and cin % 32 == 0 and width % 256 == 0, w
        else:
            assert q.in_form in (F32, SP3), w
            if has_down and q.form in (X6, EARLY) and q.in_sample == NO_SAMPLE:
                assert q.in_form == SP3, w                # the second source of conv3 is the block input's planes
        if b2b:                                            # what the loader builds these forms' weights for
            assert q.in_form == F32 and b < 7 and width in (64, 128) and SIDE[b] ** 2 >= 256, w
            assert {B2B: not has_down and stride == 1, B2BX2: has_down and (cin, width, stride) == (64, 64, 1),
                    B2BDOWN: has_down and stride == 2 and width == 128 and cin >= 256}[q.form], w
        if q.form in (EARLY, B2B, B2BX2, B2BDOWN):
            assert b < 7 and q.s_t1 >= 0 and q.s_in_max >= 0 and q.s_out >= 0, w
        if q.c1_h2:
            assert q.in_form == F32 and b < 7 and cin >= 256 and width == 128 and q.s_c1 >= 0 and q.s_t1 >= 0, w
        assert (q.s_c1 >= 0) == bool(q.c1_h2), w
        # ---- slots: nothing is read before the step that writes it (the launches in the executor's order)
        if q.form == H2FORM:
            assert q.s_in in have_scale, w
            scale(q.s_t1, q.s_in); have_max.add(q.s_t1)
            scale(q.s_t2, q.s_t1); have_max.add(q.s_t2)
            scale(q.s_out, q.s_t2, q.s_in); have_max.add(q.s_out)
        else:
            if q.c1_h2:
                scale(q.s_c1, q.s_in_max)
            if q.s_t1 >= 0:
                scale(q.s_t1, q.s_in_max)
            if q.s_t1m >= 0:
                assert b2b and q.s_t1 >= 0, w
                have_max.add(q.s_t1m)
            planes = q.s_out if q.handover else q.s_dr_out
            if b2b:
                if q.form == B2BDOWN:
                    assert q.s_dr_in in have_scale, w
                if planes >= 0:
                    scale(planes, q.s_t1m, q.s_in_max)
            else:
                assert q.s_dr_out == -1, w
                if q.handover:
                    have_max.add(q.s_t2)
                    scale(planes, q.s_t2, q.s_in_max)
            if q.s_out >= 0:
                have_max.add(q.s_out)
        # ---- the output: planes for the next block, fp32 exactly where something reads it
        assert (q.out_form == NONE) == (last and q.form == H2FORM), w
        if q.handover:
            assert b == 6 and q.out_form == H2 and q.s_out in have_scale and blocks[b + 1].form == H2FORM, w
        if q.form == H2FORM and not last:
            assert q.out_form == H2 and q.s_out in have_scale, w
        assert (q.out_form == H2) <= (q.handover or q.form == H2FORM), w
        if q.out_sample != NO_SAMPLE:
            assert b2b and q.out_form == F32 and GEOM[b + 1][4] and GEOM[b + 1][3] == 2, w
            assert (q.out_sample == SAMPLE_H2) == (q.s_dr_out >= 0) and (q.s_dr_out < 0 or q.s_dr_out in have_scale), w
        else:
            assert q.s_dr_out == -1, w
        tapped = tap >= 0
        assert q.want_mean == int(tapped and n_ls > 0) and q.want_export == int(tapped and bool(taps >> tap & 1)), w
        assert q.fuse_mean <= q.want_mean and (not q.fuse_mean or hwo % 4 == 0) and (q.fuse_mean or not q.want_mean or hwo % 4 != 0), w
        pool_tail = last and want_pool and not pool_from_stack
        every_image = q.out_form == F32 or q.want_export or pool_tail
        assert q.need32 == int(every_image or (q.want_mean and not q.fuse_mean)), w
        assert q.rows32 == (N if every_image else n_ls) * hwo, w
        assert q.no_split <= int(tapped and not b2b), w
        prev_form, prev_sample, prev = q.out_form, q.out_sample, q
    assert prev_form in (NONE, SP3)


def check_default_schedules(lib):
    """The default schedule under "gemm_precision" 3 and 2, written out (confirmed against the kernel trace of a forward on the GPU)."""
    for req in REQUESTS.values():
        stem, blocks = plan(lib, (3, 1, 1, 1, 1, 1), req)
        assert stem["conv1_h2"] == 1 and stem["pool_f32"] == 1            # the stem on f16x2, the max-pool writes fp32 rows
        assert [q.form for q in blocks] == [B2BX2, B2B, B2B, B2BDOWN, B2B, B2B, B2B] + [H2FORM] * 9
        assert blocks[2].out_sample == SAMPLE_H2 and blocks[3].in_sample == SAMPLE_H2 and blocks[3].s_dr_in == blocks[2].s_dr_out >= 0
        assert [q.c1_h2 for q in blocks] == [0, 0, 0, 1, 1, 1, 1] + [0] * 9   # layer2's conv1 (K >= 256, 128 columns)
        assert [q.out_form for q in blocks] == [F32] * 6 + [H2] * 9 + [NONE]
        stem, blocks = plan(lib, (2, 1, 1, 1, 1, 1), req)
        assert stem == dict(conv1_h2=0, pool_f32=0, s_stem=-1, n_slots=0)
        assert all(q.form == X6 and not q.c1_h2 for q in blocks)            # conv3 + downsample in one contraction on blocks 0, 3, 7, 13
        assert [b for b in range(16) if GEOM[b][4]] == [0, 3, 7, 13] and all(blocks[b].in_form == SP3 for b in (0, 3, 7, 13))
        assert [q.out_form for q in blocks] == [F32, F32, SP3, F32, F32, F32] + [SP3] * 10


def check_all(lib):
    lib.relax_host_rn_plan.restype = C.c_int
    check_geometry(lib)
    cases = 0
    for precision in (2, 3):
        for flags in itertools.product((0, 1), repeat=5):                   # rn_h2, rn_h2_early, rn_fuse, rn_c1_h2, x6_fp32_rows
            opts = (precision,) + flags
            fixed = None
            for name, req in REQUESTS.items():
                where = (opts, name)
                stem, blocks = plan(lib, opts, req)
                check_case(stem, blocks, req, where)
                # one slot too few: refused with a message, no plan
                msg = plan(lib, opts, req, stem["n_slots"] - 1)
                assert isinstance(msg, str) and "%d per-image scale slots used, %d reserved" % (stem["n_slots"], stem["n_slots"] - 1) in msg, where
                # request-independence: the launch forms, no_split, the tensors' forms and the slots do not look at the request
                shape = (stem["conv1_h2"], stem["pool_f32"], stem["s_stem"], stem["n_slots"],
                         [tuple(getattr(q, f) for f in FIELDS if f not in ("need32", "rows32", "want_mean", "fuse_mean", "want_export")) for q in blocks])
                fixed = fixed or shape
                assert shape == fixed, where
                cases += 1
            if precision == 2 or not flags[0]:
                assert stem["n_slots"] == 0 and all(q.form == X6 for q in blocks), opts
    check_default_schedules(lib)
    assert cases == 320
    return cases
