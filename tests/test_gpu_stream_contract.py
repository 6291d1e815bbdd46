"""-m gpu: the stream contract of include/relax_hip.h ("All work is enqueued on it; no hidden synchronisation"), entry by entry, on a
side stream that is HELD while the call is made.

The other GPU tests run on torch's default stream, the null stream, where a launch that lost its stream argument, a memset on stream 0
or a stray blocking copy is ordered by accident.  Here every record of tests/stream_cases.py goes through run_held():

  1. default stream: want = call(real); the call again, bit-equal; call(decoy) LAST, so every workspace holds the decoy's
     intermediates; at least one output differs between the two inputs;
  2. staged = clones of the decoy's tensors; side = a non-blocking stream that was PROBED: the null stream runs while it is held
     (side_stream(): a new stream can share the null stream's hardware queue, about one in three did here, and then hides escaped work);
  3. on `side`: a hold (torch.cuda._sleep), an event behind it, a kernel on the null stream that must finish beside the hold,
     staged <- real, outs = call(staged), `still_held` = the event has not fired when the call returns, snapshots of outs,
     staged <- decoy again;
  4. the snapshots are BIT-equal to want: work issued on any other stream runs while `side` is held, reads the decoy's input or
     workspace, and the bits differ;
  5. "enqueue" records: still_held - the call came back while its stream was blocked, so it waited for neither the stream nor the device.

Records with capture=True are then captured into a graph on a side stream and replayed on CHANGED input (decoy, then real), each
replay bit-equal to the eager result: test_step_is_graph_capturable's check, sensitive to anything the host decided from the data at
capture time.  Nothing here has a tolerance: the eager results are pinned to fp64, the oracles and Pillow by the parity modules.

The hold is max(30 ms, 3 x the call's warm host time), at most 400 ms; it is a delay, not a pass criterion.  Three fake cases written
in torch prove that the helper catches work on another stream and a wait (a hold that is too short, or a side stream that blocks
against the null stream, would make every test below pass vacuously).

measure() runs everything and returns what profiles/stream_contract.json records (tools/stream_contract_profile.py writes it).
"""
import math
import time

import pytest
import torch

from tests import stream_cases as sc

pytestmark = pytest.mark.gpu

MIN_HOLD_MS, HOLD_FACTOR, MAX_HOLD_MS = 30.0, 3.0, 400.0
ALL = {**sc.CASES, **sc.COMPOSITES}
EACH = [k for k, c in ALL.items() if c.precisions == sc.PRECISIONS]
ONCE = [k for k in ALL if k not in EACH]
TIMES = {}                 # run id -> dict(host_ms, hold_ms), for measure()
_cal, _matmul = {}, {}


# ---- the hold -----------------------------------------------------------------------------------------------------------------------
def _timed_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def calibration():
    """Once per module: the spin kernel's cycles per millisecond between two events (or, without torch.cuda._sleep, the time of one
    large matmul of a chain)."""
    if _cal:
        return _cal
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(100_000)                                   # the kernel's first launch
        probe = 2_000_000
        ms = _timed_ms(lambda: torch.cuda._sleep(probe))
        probe = max(int(probe * 20.0 / max(ms, 1e-3)), 1000)       # a second probe of about 20 ms
        ms = _timed_ms(lambda: torch.cuda._sleep(probe))
        _cal.update(mode="torch.cuda._sleep", probe_cycles=probe, probe_ms=ms, cycles_per_ms=probe / ms)
    else:
        _matmul["a"] = torch.randn(4096, 4096, device="cuda")
        _matmul["b"] = torch.empty_like(_matmul["a"])
        torch.mm(_matmul["a"], _matmul["a"], out=_matmul["b"])
        ms = _timed_ms(lambda: [torch.mm(_matmul["a"], _matmul["a"], out=_matmul["b"]) for _ in range(16)])
        _cal.update(mode="matmul chain 4096^3", probe_matmuls=16, probe_ms=ms, ms_per_matmul=ms / 16)
    return _cal


def hold(ms):
    """Keeps the current stream busy for about `ms` milliseconds: a bounded delay, enqueued, never waited for here."""
    cal = calibration()
    if "cycles_per_ms" in cal:
        torch.cuda._sleep(int(ms * cal["cycles_per_ms"]))
    else:
        for _ in range(int(math.ceil(ms / cal["ms_per_matmul"]))):
            torch.mm(_matmul["a"], _matmul["a"], out=_matmul["b"])


# ---- the side stream ----------------------------------------------------------------------------------------------------------------
SIDE_PROBE_MS, SIDE_CANDIDATES = 20.0, 32
_side = {}


def side_stream():
    """A non-blocking stream beside which the null stream demonstrably RUNS while it is held.  The runtime maps its streams onto a few
    hardware queues (four by default); a stream that shares the null stream's queue serialises the null stream's work behind the hold,
    and escaped work would then read the staged input after all - the run would pass vacuously.  Which streams collide depends on how
    many the process has made before, i.e. on the tests that ran earlier.  So candidates are probed, once per module: a hold on the
    candidate, a small kernel and an event on the null stream, and the candidate is taken if that event fires while the hold is still
    on.  Bounded: at most SIDE_CANDIDATES probes of SIDE_PROBE_MS each."""
    if "stream" in _side:
        return _side["stream"]
    probe, tried = torch.zeros(64, device="cuda"), []
    for _ in range(SIDE_CANDIDATES):
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        held, done = torch.cuda.Event(), torch.cuda.Event()
        with torch.cuda.stream(s):
            hold(SIDE_PROBE_MS)
            held.record()
        with torch.cuda.stream(torch.cuda.default_stream()):
            probe.add_(1)
            done.record()
        done.synchronize()                      # returns at once beside the hold, after it (20 ms) behind it
        independent = not held.query()
        torch.cuda.synchronize()
        tried.append(independent)
        if independent:
            _side.update(stream=s, probes=tried, probe=probe)
            return s
    raise AssertionError(f"none of {SIDE_CANDIDATES} new streams ran beside the null stream: {tried}")


# ---- the held-stream run ------------------------------------------------------------------------------------------------------------
def bits_equal(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def _all_equal(xs, ys):
    return len(xs) == len(ys) and all(bits_equal(x, y) for x, y in zip(xs, ys))


def _call(case, eng, inputs):
    if case.prepare is not None:
        case.prepare(eng, inputs)            # waits for the device by contract: never inside a hold or a capture
    return tuple(case.call(eng, inputs))


class Report:
    """What run_held saw: mismatch = indices of the outputs whose bits differ from the default-stream result; still_held = the call
    returned while its stream was blocked."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _poison_off(fn):
    """debug_poison fills workspaces synchronously by design: read it, run with 0, restore it"""
    def wrapped(case, *a, **k):
        eng = sc.ensure(case.needs)
        poison = eng.get_option("debug_poison")
        eng.set_option("debug_poison", 0)
        try:
            return fn(case, eng, *a, **k)
        finally:
            eng.set_option("debug_poison", poison)
    return wrapped


@_poison_off
def run_held(case, eng, run_id):
    real, decoy = case.make(sc.REAL), case.make(sc.DECOY)
    assert real.keys() == decoy.keys()
    want = _call(case, eng, real)
    torch.cuda.synchronize()
    if case.prepare is not None:
        case.prepare(eng, real)
    t0 = time.perf_counter()
    again = tuple(case.call(eng, real))
    host_ms = (time.perf_counter() - t0) * 1e3
    assert _all_equal(want, again), f"{run_id}: two calls on the default stream differ"
    decoy_out = _call(case, eng, decoy)                     # LAST: the workspaces now hold the decoy's intermediates
    torch.cuda.synchronize()
    assert len(want) == len(decoy_out) and not _all_equal(want, decoy_out), f"{run_id}: the decoy input gives the real input's outputs"
    hold_ms = max(MIN_HOLD_MS, HOLD_FACTOR * host_ms)
    TIMES[run_id] = {"host_ms": round(host_ms, 3), "hold_ms": round(hold_ms, 3)}
    assert hold_ms <= MAX_HOLD_MS, f"{run_id}: a hold of {hold_ms:.0f} ms: the case is too large, shrink its shape"
    staged = {k: v.clone() for k, v in decoy.items()}
    if case.prepare is not None:
        case.prepare(eng, real)
    torch.cuda.synchronize()
    side = side_stream()                                    # non-blocking, and not on the null stream's hardware queue
    with torch.cuda.stream(side):
        hold(hold_ms)
        held = torch.cuda.Event()
        held.record()
        with torch.cuda.stream(torch.cuda.default_stream()):      # every run checks it again: the null stream runs beside this hold
            _side["probe"].add_(1)
            beside = torch.cuda.Event()
            beside.record()
        beside.synchronize()
        assert not held.query(), f"{run_id}: the null stream ran only after the side stream's hold: this run could not see escaped work"
        for k in staged:
            staged[k].copy_(real[k])
        outs = tuple(case.call(eng, staged))
        still_held = not held.query()
        snap = [o.clone() for o in outs]
        for k in staged:
            staged[k].copy_(decoy[k])                       # escaped work that runs late reads the wrong data too
    side.synchronize()
    torch.cuda.synchronize()
    mismatch = [i for i, (s, w) in enumerate(zip(snap, want)) if not bits_equal(s, w)] if len(snap) == len(want) else ["count"]
    return Report(mismatch=mismatch, still_held=still_held, host_ms=host_ms, hold_ms=hold_ms, want=want, decoy_out=decoy_out, real=real,
                  decoy=decoy)


def check_held(key, run_id=None):
    case, run_id = ALL[key], run_id or key
    rep = run_held(case, run_id)
    print(f"{run_id}: host {rep.host_ms:.2f} ms, hold {rep.hold_ms:.0f} ms, still held on return: {rep.still_held}, outputs off: {rep.mismatch}")
    assert not rep.mismatch, f"{run_id}: outputs {rep.mismatch} on the held side stream differ from the default stream's: work left the caller's stream"
    if case.kind == "enqueue":
        assert rep.still_held, f"{run_id}: the call returned only after its stream's hold ({rep.hold_ms:.0f} ms) had run out: it waited"
    return rep


# ---- capture, replay on changed input -----------------------------------------------------------------------------------------------
@_poison_off
def run_capture(case, eng, run_id, rep):
    """rep: run_held's report of the same case (the no-wait check is made BEFORE any capture begins)"""
    assert rep.still_held and not rep.mismatch, f"{run_id}: not captured, the held-stream run did not pass"
    staged = {k: v.clone() for k, v in rep.real.items()}
    side = torch.cuda.Stream()
    if case.prepare is not None:
        case.prepare(eng, staged)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        case.call(eng, staged)                              # warm on the capturing stream
    torch.cuda.synchronize()
    if case.prepare is not None:
        case.prepare(eng, staged)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):              # single stream, linear
            outs = tuple(case.call(eng, staged))
    torch.cuda.synchronize()
    for name, inputs, expect in (("decoy", rep.decoy, rep.decoy_out), ("real", rep.real, rep.want)):
        if case.prepare is not None:
            case.prepare(eng, inputs)
        for o in outs:
            o.zero_()
        for k in staged:
            staged[k].copy_(inputs[k])
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        off = [i for i, (o, w) in enumerate(zip(outs, expect)) if not bits_equal(o, w)]
        assert len(outs) == len(expect) and not off, f"{run_id}: replay on the {name} input: outputs {off} differ from the eager result"


def check_capture(key, run_id=None):
    run_id = run_id or key
    run_capture(ALL[key], run_id, check_held(key, run_id))


# ---- self-test of the helper: three fakes in torch, no library code -----------------------------------------------------------------
def _fake_make(seed):
    return {"x": torch.arange(1 << 16, device="cuda", dtype=torch.float32) * seed}


def _fake_good(eng, t):
    return (t["x"] * 2 + 1,)


def _fake_other_stream(eng, t):
    with torch.cuda.stream(torch.cuda.default_stream()):
        return (t["x"] * 2 + 1,)


def _fake_waits(eng, t):
    out = t["x"] * 2 + 1
    torch.cuda.current_stream().synchronize()
    return (out,)


FAKES = {"good": sc.Case("enqueue", _fake_make, _fake_good), "other_stream": sc.Case("enqueue", _fake_make, _fake_other_stream),
         "waits": sc.Case("enqueue", _fake_make, _fake_waits)}


def selftest():
    """-> {fake: (mismatch, still_held)}; asserts that the helper tells the three apart"""
    seen = {}
    for name, case in FAKES.items():
        rep = run_held(case, "fake:" + name)
        seen[name] = (bool(rep.mismatch), rep.still_held)
    assert seen["good"] == (False, True), f"a well-behaved call does not pass: {seen}"
    assert seen["other_stream"][0], f"work on the default stream went unnoticed (is the side stream blocking, or the hold too short?): {seen}"
    assert seen["waits"] == (False, False), f"a call that waits for its stream went unnoticed (hold too short?): {seen}"
    return seen


def test_helper_passes_a_well_behaved_call_and_catches_the_two_misbehaving_ones():
    print(calibration(), selftest())


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def _module_wall_time():
    t0 = time.perf_counter()
    yield
    print(f"\nstream contract module: {time.perf_counter() - t0:.1f} s")


@pytest.mark.parametrize("key", ONCE)
def test_held_stream(key):
    case = ALL[key]
    if case.precisions:
        sc.ensure(()).set_precision(case.precisions[0])
    (check_capture if case.capture else check_held)(key)


@pytest.mark.parametrize("key", EACH)
def test_held_stream_each_precision(key, each_precision):
    (check_capture if ALL[key].capture else check_held)(key, f"{key}[{each_precision}]")


# ---- what profiles/stream_contract.json records -------------------------------------------------------------------------------------
def _gpu_trouble(e):
    text = str(e).lower()
    return isinstance(e, RuntimeError) and any(w in text for w in ("hip", "illegal", "memory access", "failed (-2)", "device-side"))


def measure():
    """Every case under every precision through the helpers the tests call; a failing case is recorded, not raised (a HIP error ends
    the run: nothing more is started on the device after one)."""
    t0 = time.perf_counter()
    eng = sc.ensure(())
    side_stream()
    out = {"calibration": dict(calibration()), "side_stream_probes": list(_side["probes"]), "hold_rule": f"max({MIN_HOLD_MS:g} ms, {HOLD_FACTOR:g} x warm host time), at most {MAX_HOLD_MS:g} ms",
           "selftest": {k: {"bit_mismatch": v[0], "still_held": v[1]} for k, v in selftest().items()}, "cases": {}}
    stopped = None
    for key, case in ALL.items():
        for prec in case.precisions or (None,):
            run_id = f"{key}[{prec}]" if case.precisions == sc.PRECISIONS else key
            eng.set_precision(prec or "f16x2")
            entry = {"kind": case.kind}
            t1 = time.perf_counter()
            try:
                rep = run_held(case, run_id)
                entry.update(bits_equal=not rep.mismatch, still_held=rep.still_held)
                if case.capture:
                    run_capture(case, run_id, rep)
                    entry["captured"] = True
            except Exception as e:          # noqa: BLE001 - recorded
                entry["error"] = f"{type(e).__name__}: {e}"[:600]
                if _gpu_trouble(e):
                    stopped = run_id
            entry.update(TIMES.get(run_id, {}), case_s=round(time.perf_counter() - t1, 2))
            out["cases"][run_id] = entry
            print(run_id, entry, flush=True)
            if stopped:
                break
        if stopped:
            break
    if not stopped:
        eng.set_precision("f16x2")
    out.update(stopped_at=stopped, held=sorted(sc.CASES), held_entries=sorted({sc.entry_of(k) for k in sc.CASES}), composites=sorted(sc.COMPOSITES),
               captured=sorted(k for k, c in ALL.items() if c.capture), exempt=dict(sc.EXEMPT), wall_s=round(time.perf_counter() - t0, 1))
    return out
