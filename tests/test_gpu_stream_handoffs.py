"""-m gpu: the cross-stream handoffs of the Python layer under contention - PinnedClipFeeder and ClipStager (a copy stream ordered
against the compute stream by `ready` / `free` events, memory kept alive across streams by record_stream), PngDecoder, PngEncoder,
GpuFrameLoader and GpuYuvLoader (each owns a stream, takes the caller's inputs with wait_stream(caller) and hands results over by a
host wait plus record_stream(consumer)).  The follow-up of tests/test_gpu_stream_contract.py, with its method and its helpers (hold,
calibration, bits_equal and the hold constants are imported, not copied).

Without contention every one of these orderings holds by accident: the copy has landed before the compute starts, the compute has
finished before the slot is reused.  So each scenario of tests/stream_handoff_cases.py

  * takes the stream of the class under test and a second stream from beside(owned): probed to RUN while `owned` is held;
  * puts a hold on the stream that should be waited for, decoy (or an earlier batch's) bytes where stale data would be read, and
    compares bits, pointers or the stager's books;
  * repeats the probe inside its own hold: a run in which the held event had fired by then is reported as vacuous and fails.

Scenarios 1, 2, 4, 5 and 8 run once more with torch.cuda.Stream.wait_event doing nothing, scenario 7 with torch.Tensor.record_stream
doing nothing, and must then REPORT a mismatch: they can fail.  So do 11 and 14 (wait_stream is a wait_event) and 13 (record_stream).
The broken variants only read stale bytes of live allocations.

measure() runs everything and returns what profiles/stream_handoffs.json records (tools/stream_handoffs_profile.py writes it)."""
import time

import pytest
import torch

from tests import stream_handoff_cases as hc
from tests.test_gpu_stream_contract import MAX_HOLD_MS

pytestmark = pytest.mark.gpu


def check(name, rep):
    print(f"{name}: {rep}")
    assert not rep.vacuous, f"{name}: the held event had fired when the other stream's probe finished: this run could not see a missing ordering"
    assert rep.hold_ms < MAX_HOLD_MS
    assert not rep.mismatch, f"{name}: {rep.mismatch}"
    return rep


def check_caught(name, rep):
    print(f"{name} (ordering removed): {rep}")
    assert not rep.vacuous, f"{name}: vacuous run"
    assert rep.mismatch, f"{name}: the ordering was removed and the scenario saw nothing"
    return rep


@pytest.fixture(scope="module", autouse=True)
def _module_wall_time():
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print(f"\nstream handoffs module: {time.perf_counter() - t0:.1f} s")


# ---- PinnedClipFeeder -------------------------------------------------------------------------------------------------------------------
def test_01_feeder_compute_waits_for_the_held_copy():
    check("feeder copy -> compute", hc.feeder_copy_to_compute())


def test_02_feeder_copy_waits_for_the_held_compute_before_it_reuses_a_slot():
    check("feeder compute -> reuse", hc.feeder_compute_to_reuse())


def test_03_feeder_primed_run_and_second_run_under_both_holds():
    check("feeder primed + second run", hc.feeder_primed_and_second_run())


# ---- ClipStager -------------------------------------------------------------------------------------------------------------------------
def test_04_stager_compute_waits_for_the_held_copy():
    check("stager copy -> compute", hc.stager_copy_to_compute())


def test_05_stager_copy_waits_for_the_held_compute_before_it_reuses_a_slot():
    check("stager compute -> reuse", hc.stager_compute_to_reuse())


def test_06_stager_keeps_a_pinned_buffer_until_its_copy_has_landed():
    check("stager pinned staging", hc.stager_pinned_staging())


def test_07_stager_old_block_of_a_grown_slot_is_kept_for_the_compute_stream():
    rep = check("stager slot growth", hc.stager_slot_growth())
    assert not rep.reused, "copy_stream got the old block back while the compute stream was held"


# ---- extract_dataset_clips --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heavy", ["copy", "compute"])
def test_08_host_clip_pass_under_contention_equals_the_inline_pass(heavy):
    rep = check(f"host-clip pass [{heavy}]", hc.dataset_pass("host", heavy))
    assert rep.grown and [i for i, _ in rep.errors] == [hc.ERROR_CLIP, hc.REFUSED_CLIP]


@pytest.mark.parametrize("heavy", ["copy", "compute"])
def test_09_alloc_loader_pass_under_contention_equals_the_inline_pass(heavy):
    rep = check(f"alloc-loader pass [{heavy}]", hc.dataset_pass("alloc", heavy))
    assert rep.grown and [i for i, _ in rep.errors] == [hc.ERROR_CLIP, hc.REFUSED_CLIP]


@pytest.mark.parametrize("kind", ["png", "yuv"])
def test_10_gpu_loader_pass_under_contention_equals_the_host_twin_pass(kind, tmp_path):
    rep = check(f"{kind} loader pass", hc.dataset_pass(kind, "compute", tmp_path))
    assert [i for i, _ in rep.errors] == [hc.ERROR_CLIP, hc.REFUSED_CLIP]


# ---- PngDecoder, GpuFrameLoader, GpuYuvLoader, PngEncoder -------------------------------------------------------------------------------
def test_11_decoder_takes_out_behind_the_held_caller():
    check("decoder inputs behind the caller", hc.decoder_inputs_behind_the_caller())


@pytest.mark.parametrize("name", hc.LOADER_CASES)
def test_12_result_is_complete_when_the_call_returns(name, tmp_path):
    check(f"complete on return: {name}", hc.complete_on_return(name, tmp_path))


@pytest.mark.parametrize("name", hc.LOADER_CASES)
def test_13_result_lives_on_while_the_held_consumer_reads_it(name, tmp_path):
    check(f"lifetime on the consumer: {name}", hc.lifetime_on_the_consumer(name, tmp_path))


@pytest.mark.parametrize("layout", hc.ENCODER_CASES)
def test_14_encoder_takes_images_behind_the_held_caller(layout):
    check(f"encoder images behind the caller: {layout}", hc.encoder_images_behind_the_caller(layout))


# ---- the scenarios can fail -------------------------------------------------------------------------------------------------------------
BROKEN = {
    "01 feeder copy -> compute": ("wait_event", lambda tmp: hc.feeder_copy_to_compute()),
    "02 feeder compute -> reuse": ("wait_event", lambda tmp: hc.feeder_compute_to_reuse()),
    "04 stager copy -> compute": ("wait_event", lambda tmp: hc.stager_copy_to_compute()),
    "05 stager compute -> reuse": ("wait_event", lambda tmp: hc.stager_compute_to_reuse()),
    "07 stager slot growth": ("record_stream", lambda tmp: hc.stager_slot_growth()),
    "08 host-clip pass [copy]": ("wait_event", lambda tmp: hc.dataset_pass("host", "copy")),
    "08 host-clip pass [compute]": ("wait_event", lambda tmp: hc.dataset_pass("host", "compute")),
    # beyond the six the method asks for: wait_stream(caller) is a wait_event, and the results' lifetime is a record_stream
    "11 decoder inputs behind the caller": ("wait_event", lambda tmp: hc.decoder_inputs_behind_the_caller()),
    **{f"13 lifetime on the consumer: {n}": ("record_stream", lambda tmp, n=n: hc.lifetime_on_the_consumer(n, tmp)) for n in hc.LOADER_CASES},
    "14 encoder images behind the caller: contiguous": ("wait_event", lambda tmp: hc.encoder_images_behind_the_caller("contiguous")),
    "14 encoder images behind the caller: strided": ("wait_event", lambda tmp: hc.encoder_images_behind_the_caller("strided")),
}


@pytest.mark.parametrize("name", list(BROKEN))
def test_scenario_reports_a_mismatch_when_its_ordering_is_removed(name, monkeypatch, tmp_path):
    what, scenario = BROKEN[name]
    hc.remove_ordering(monkeypatch, what)
    rep = check_caught(name, scenario(tmp_path))
    if name.startswith("07"):
        assert rep.reused and "small clip" in rep.mismatch
    if name.startswith("13"):
        assert "the second result lies in the first's storage" in rep.mismatch and "held clone" in rep.mismatch


# ---- what profiles/stream_handoffs.json records -------------------------------------------------------------------------------------------
def scenarios(tmp_path):
    out = {
        "01 feeder copy -> compute": hc.feeder_copy_to_compute, "02 feeder compute -> reuse": hc.feeder_compute_to_reuse,
        "03 feeder primed + second run": hc.feeder_primed_and_second_run, "04 stager copy -> compute": hc.stager_copy_to_compute,
        "05 stager compute -> reuse": hc.stager_compute_to_reuse, "06 stager pinned staging": hc.stager_pinned_staging,
        "07 stager slot growth": hc.stager_slot_growth,
        "08 host-clip pass [copy]": lambda: hc.dataset_pass("host", "copy"), "08 host-clip pass [compute]": lambda: hc.dataset_pass("host", "compute"),
        "09 alloc-loader pass [copy]": lambda: hc.dataset_pass("alloc", "copy"), "09 alloc-loader pass [compute]": lambda: hc.dataset_pass("alloc", "compute"),
        "10 png loader pass": lambda: hc.dataset_pass("png", "compute", tmp_path), "10 yuv loader pass": lambda: hc.dataset_pass("yuv", "compute", tmp_path),
        "11 decoder inputs behind the caller": hc.decoder_inputs_behind_the_caller,
    }
    for n in hc.LOADER_CASES:
        out[f"12 complete on return: {n}"] = lambda n=n: hc.complete_on_return(n, tmp_path)
    for n in hc.LOADER_CASES:
        out[f"13 lifetime on the consumer: {n}"] = lambda n=n: hc.lifetime_on_the_consumer(n, tmp_path)
    for n in hc.ENCODER_CASES:
        out[f"14 encoder images behind the caller: {n}"] = lambda n=n: hc.encoder_images_behind_the_caller(n)
    return out


def measure(tmp_path):
    """Every scenario, and the broken variant of those that have one, through the functions the tests call; a failing scenario is
    recorded, not raised (a HIP error ends the run: nothing more is started on the device after one)."""
    from tests.test_gpu_stream_contract import HOLD_FACTOR, MIN_HOLD_MS, _gpu_trouble, calibration
    t0 = time.perf_counter()
    out = {"calibration": dict(calibration()), "hold_rule": f"max({MIN_HOLD_MS:g} ms, {HOLD_FACTOR:g} x warm host time), at most {MAX_HOLD_MS:g} ms; "
           "the dataset passes hold one stream three times as long as the other", "scenarios": {}, "stopped_at": None}
    for name, fn in scenarios(tmp_path).items():
        entry = {}
        t1 = time.perf_counter()
        try:
            rep = fn()
            entry.update(host_ms=round(rep.host_ms, 3), hold_ms=round(rep.hold_ms, 3), beside_tried=rep.tried, vacuous=bool(rep.vacuous),
                         passed=not rep.mismatch and not rep.vacuous)
            if name in BROKEN:
                with hc.ordering_removed(BROKEN[name][0]):
                    bad = BROKEN[name][1](tmp_path)
                entry.update(ordering_removed=BROKEN[name][0], broken_variant_caught=bool(bad.mismatch) and not bad.vacuous)
        except Exception as e:          # noqa: BLE001 - recorded
            entry["error"] = f"{type(e).__name__}: {e}"[:600]
            if _gpu_trouble(e):
                out["stopped_at"] = name
        entry["scenario_s"] = round(time.perf_counter() - t1, 2)
        out["scenarios"][name] = entry
        print(name, entry, flush=True)
        if out["stopped_at"]:
            break
    out["wall_s"] = round(time.perf_counter() - t0, 1)
    return out
