"""Inputs, the stand-in engine and the scenarios of tests/test_gpu_stream_handoffs.py: the cross-stream handoffs of the Python layer
(feeder.PinnedClipFeeder, dataset.ClipStager / extract_dataset_clips, pngdecode.PngDecoder, pngencode.PngEncoder,
sampling.GpuFrameLoader / GpuYuvLoader).  Each of these classes owns a stream and orders it against the caller's with events, a host wait
or record_stream; a missing one raises nothing and faults nothing - a clip is computed from the previous batch's bytes.

The method is the stream contract test's (tests/test_gpu_stream_contract.py): a bounded hold() on the stream that should be waited for,
decoy bytes where stale data would be read, bit-equality, and a probe that the two streams really run beside each other.  Every scenario
below is a function -> Report:

  mismatch   what differed from the expected bytes / pointers / books (empty: the handoff held)
  vacuous    the held event had fired before the other stream's probe finished: the run could not have seen a missing ordering
  host_ms    warm host time of the phase the hold must outlast;  hold_ms: the (longest) hold;  tried: candidates beside() probed

Nothing here has a tolerance.  The module imports without a GPU: the CPU test of the inputs and the stand-in engine uses it too."""
import contextlib
import io
import itertools
import time

import numpy as np
import pytest
import torch

from relax_vqa_amd import dataset, feeder, pngdecode, pngencode, sampling
from tests.test_gpu_stream_contract import (HOLD_FACTOR, MAX_HOLD_MS, MIN_HOLD_MS, SIDE_CANDIDATES, SIDE_PROBE_MS, bits_equal,
                                            calibration, hold)

# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
REAL, DECOY = 1, 2
REFUSED_HW = (40, 40)                  # the stand-in engine refuses clips of this frame size (known without reading a device byte)
ERROR_CLIP, REFUSED_CLIP, GROWTH_BATCH = 3, 6, 2
# the ragged set of the dataset passes, two clips per batch; slot 0 takes batches 0, 2, 4 and slot 1 batches 1, 3:
#   batch 0  two small clips: slot 0 becomes a block of 2 x 6144 bytes
#   batch 1  clip 3 cannot be loaded
#   batch 2  a small clip that fits the block, then one that does not: the slot grows inside the batch
#   batch 3  clip 6 is refused by the engine: the batch is retried clip by clip, and clip 7 is read late
RAGGED = [(1, 2, 32, 32, 3), (1, 2, 32, 32, 3),
          (2, 2, 32, 48, 3), None,
          (1, 2, 32, 32, 3), (3, 2, 64, 64, 3),
          (2, 2) + REFUSED_HW + (3,), (2, 2, 48, 32, 3),
          (3, 2, 32, 64, 3), (1, 2, 64, 32, 3)]
FEEDER_SHAPES = [(2, 2, 32, 48, 3), (3, 2, 40, 32, 3)]       # clip j of every step has shape j
FEEDER_STEPS = 4
PNG_HW, PNG_HW_OTHER = (48, 64), (40, 56)
YUV_W, YUV_H = 48, 32


def clip_bytes(shape, seed, which=REAL):
    """uint8 ndarray of `shape`: random bytes, different for every (seed, which)."""
    return np.random.default_rng([int(seed), int(which), 20251]).integers(0, 256, shape, dtype=np.uint8)


def ragged_clips(which=REAL, salt=0):
    """-> list of ndarrays (None at ERROR_CLIP); salt: other bytes, same shapes"""
    return [None if s is None else clip_bytes(s, 100 + i + 1000 * salt, which) for i, s in enumerate(RAGGED)]


def slot_blocks(shapes, per_batch):
    """What ClipStager.add does to a slot over a pass, on the host: -> [(batch, clip in batch)] where a block is replaced although the
    batch has copied into it already (growth INSIDE a batch).  The rule: a clip takes ceil(bytes / 256) * 256; a block that is too
    small is replaced by one of (clips still to come in the batch) x (this clip's size)."""
    blocks, grown = [0, 0], []
    for b in range(0, len(shapes), per_batch):
        slot, at, left = (b // per_batch) & 1, 0, per_batch
        for j, s in enumerate(shapes[b:b + per_batch]):
            if s is None:
                continue
            sz = -(-int(np.prod(s)) // 256) * 256
            if at + sz > blocks[slot]:
                if at > 0:
                    grown.append((b // per_batch, j))
                blocks[slot], at = left * sz, 0
            at += sz
            left = max(left - 1, 1)
    return grown


# ---- the fingerprint and the stand-in engine --------------------------------------------------------------------------------------------
FP_DIM = 9
FP_MAX_BYTES = (1 << 36) // (255 * 251)


def fingerprint(clip):
    """Every byte of `clip` -> 9 fp32 values, exact: three int64 sums (the bytes; the bytes weighted 1 + k % 251; weighted
    1 + (k // 251) % 241), each below 2^36, cut into 12-bit pieces.  The plain sum changes with any single-byte change; the weighted
    sums tell apart clips that hold the same bytes in another order.  Torch ops on the clip's device, on the current stream."""
    x = clip.reshape(-1).to(torch.int64)
    assert x.numel() <= FP_MAX_BYTES
    k = torch.arange(x.numel(), device=x.device, dtype=torch.int64)
    sums = torch.stack([x.sum(), (x * (1 + k % 251)).sum(), (x * (1 + (k // 251) % 241)).sum()])
    pieces = torch.stack([(sums >> (12 * j)) & 0xFFF for j in range(3)], dim=1)
    return pieces.reshape(-1).to(torch.float32)


class FingerprintEngine:
    """What extract_dataset_clips needs of an engine; a clip's row is its fingerprint.  A clip of REFUSED_HW raises, as a failing
    engine call takes a whole batch down.  With hold_ms = (compute, copy) every call first holds the current stream, then computes,
    then holds `copy_stream` - so the next batch's copies run late and this batch's reads run late.  The first held call checks that
    `copy_stream` runs beside the held compute stream (vacuous)."""
    vit_dim = None

    def __init__(self, device, hold_ms=None, copy_stream=None):
        self.device = torch.device(device)
        self.hold_ms, self.copy_stream = hold_ms, copy_stream
        self.calls, self.vacuous = 0, None

    def rows_mean(self, rows):
        return rows.mean(dim=0)

    def clip_vectors(self, clips, resnet=True, vit=True, per_frame=False):
        self.calls += 1
        if self.hold_ms:
            hold(self.hold_ms[0])
            if self.vacuous is None:
                held = torch.cuda.Event()
                held.record()
                self.vacuous = not runs_beside(held, self.copy_stream)
        for c in clips:
            if tuple(c.shape[2:4]) == REFUSED_HW:
                raise RuntimeError(f"relax_fragment_pairs failed (-2): refused a clip of {tuple(c.shape)}")
        out = torch.stack([fingerprint(c.to(self.device)) for c in clips])
        if self.hold_ms:
            with torch.cuda.stream(self.copy_stream):
                hold(self.hold_ms[1])
        return out


@contextlib.contextmanager
def fingerprint_width():
    """dataset.feature_dim is the stand-in's width while a pass runs (restored afterwards: other tests share the session)"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(dataset, "feature_dim", lambda engine, resnet=True, vit=True, full=False: FP_DIM)
        yield


def host_source(which=REAL, alloc=False, salt=0):
    """-> clips(i) over ragged_clips(): pageable host tensors, or (alloc) decoded into the array the driver's `alloc` hands out"""
    data = ragged_clips(which, salt)

    def plain(i):
        if data[i] is None:
            raise OSError(f"cannot decode clip {i}")
        return torch.from_numpy(data[i].copy())

    def into(i, alloc=None):
        if data[i] is None:
            raise OSError(f"cannot decode clip {i}")
        out = alloc(data[i].shape) if alloc is not None else np.empty(data[i].shape, np.uint8)
        out[...] = data[i]
        return out
    return into if alloc else plain


def run_pass(clips, engine, **kw):
    with fingerprint_width():
        return dataset.extract_dataset_clips(clips, len(RAGGED), engine, clips_per_step=2, rank=0, world=1, **kw)


# ---- files ------------------------------------------------------------------------------------------------------------------------------
def png_bytes(bgr):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(buf, format="PNG", compress_level=3)
    return buf.getvalue()


def write_png_clips(d, which=REAL):
    """ragged_clips() as `v<i>_<12 t>.png` / `v<i>_<12 t>_next.png` under d (no file for ERROR_CLIP) -> names"""
    d.mkdir(parents=True, exist_ok=True)
    for i, c in enumerate(ragged_clips(which)):
        for t in range(0 if c is None else c.shape[0]):
            (d / f"v{i}_{12 * t}.png").write_bytes(png_bytes(c[t, 0]))
            (d / f"v{i}_{12 * t}_next.png").write_bytes(png_bytes(c[t, 1]))
    return [f"v{i}" for i in range(len(RAGGED))]


def write_yuv_clips(d, which=REAL):
    """One raw yuv420p file per clip of RAGGED, of 12 (T - 1) + 2 frames (T pairs at framerate 25); one frame - no pair - for
    ERROR_CLIP -> (paths, widths, heights)"""
    d.mkdir(parents=True, exist_ok=True)
    paths, widths, heights = [], [], []
    for i, s in enumerate(RAGGED):
        T, H, W = (1, YUV_H, YUV_W) if s is None else (s[0], s[2], s[3])
        fb = sampling.yuv_frame_bytes(sampling.yuv_layout("yuv420p")[0], H, W)
        n = 1 if s is None else 12 * (T - 1) + 2
        p = d / f"v{i}.yuv"
        clip_bytes((n, fb), 300 + i, which).tofile(str(p))
        paths.append(str(p)), widths.append(W), heights.append(H)
    return paths, widths, heights


# ---- holds, probes, reports -------------------------------------------------------------------------------------------------------------
class Report:
    def __init__(self, **kw):
        self.__dict__.update(mismatch=[], vacuous=False, host_ms=0.0, hold_ms=0.0, tried=0)
        self.__dict__.update(kw)

    def __repr__(self):
        return (f"host {self.host_ms:.2f} ms, hold {self.hold_ms:.0f} ms, beside() tried {self.tried}, vacuous: {self.vacuous}, "
                f"off: {self.mismatch}" + (f" ({self.notes})" if getattr(self, "notes", None) else ""))


def device():
    return torch.device("cuda", torch.cuda.current_device())


def hold_for(host_ms, factor=1.0):
    """The contract test's rule; factor: the long hold of a scenario whose two streams must lag by different amounts."""
    ms = factor * max(MIN_HOLD_MS, HOLD_FACTOR * host_ms)
    assert ms <= MAX_HOLD_MS, f"a hold of {ms:.0f} ms: the scenario is too large, shrink its inputs"
    return ms


def ms_of(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


_probe = {}


def runs_beside(held, other):
    """A small kernel and an event on `other`, waited for on the host -> True if `held` (an event behind a hold on another stream)
    has not fired by then: `other` ran while that stream was blocked."""
    if "t" not in _probe:
        _probe["t"] = torch.zeros(64, device=device())
    done = torch.cuda.Event()
    with torch.cuda.stream(other):
        _probe["t"].add_(1)
        done.record()
    done.synchronize()
    return not held.query()


def held_event(stream, ms):
    """hold(ms) on `stream` and an event behind it"""
    ev = torch.cuda.Event()
    with torch.cuda.stream(stream):
        hold(ms)
        ev.record()
    return ev


def snap(t, out=None):
    """A copy of `t` made by a kernel on the current stream, as an engine's read of a clip is one.  (clone() / copy_() may be routed to a
    DMA engine whose queue the copies of other streams share; whether a held stream's copy then delays them was not measured, and no
    scenario should depend on it.)"""
    return torch.add(t, 0, out=out)


TRIED = []


def beside(owned, *others):
    """A new non-blocking stream that demonstrably runs while `owned` is held: side_stream()'s probe with the held stream as a
    parameter (new streams come from a small pool and are mapped onto a few hardware queues: a candidate may BE `owned` or share its
    queue, and a scenario on it would pass whatever the code does).  others: streams the scenario's calls touch besides - the null
    stream, where a loader is called from a thread's default stream: its wait_stream(caller) puts an event there, and behind a hold on
    a stream that shares the null stream's queue that event - and so the whole call - waits for the hold.  The candidate runs beside
    each of them.  At most SIDE_CANDIDATES candidates, one probe of SIDE_PROBE_MS per stream."""
    calibration()
    tried = []
    for _ in range(SIDE_CANDIDATES):
        s = torch.cuda.Stream(device())
        ok = s != owned
        for x in (owned,) + others:
            torch.cuda.synchronize()
            ok = ok and runs_beside(held_event(x, SIDE_PROBE_MS), s)
        torch.cuda.synchronize()
        tried.append(ok)
        if ok:
            TRIED.append(len(tried))
            return s
    raise AssertionError(f"none of {SIDE_CANDIDATES} new streams ran beside the held stream: {tried}")


@contextlib.contextmanager
def ordering_removed(what):
    """The broken variants: torch.cuda.Stream.wait_event (and with it wait_stream) or torch.Tensor.record_stream does nothing.  A copy
    or a clone then reads stale bytes of live allocations; nothing is launched on freed memory."""
    with pytest.MonkeyPatch.context() as mp:
        remove_ordering(mp, what)
        yield


def remove_ordering(mp, what):
    if what == "wait_event":
        mp.setattr(torch.cuda.Stream, "wait_event", lambda self, event: None)
    elif what == "record_stream":
        mp.setattr(torch.Tensor, "record_stream", lambda self, stream: None)
    else:
        raise ValueError(what)


def _off(got, want, tag):
    want = torch.as_tensor(want)
    return [] if bits_equal(got.cpu(), want) else [tag]


# ---- PinnedClipFeeder (scenarios 1 - 3) -------------------------------------------------------------------------------------------------
def _feeder_inputs():
    n = 2 * FEEDER_STEPS
    real = [torch.from_numpy(clip_bytes(FEEDER_SHAPES[i % 2], i, REAL)).pin_memory() for i in range(n)]
    decoy = [torch.from_numpy(clip_bytes(FEEDER_SHAPES[j], 50 + j, DECOY)) for j in range(2)]
    return real, decoy


def _feeder_fill(f, decoy):
    for slot in f.buffers:
        for b, d in zip(slot, decoy):
            b.copy_(d)
    torch.cuda.synchronize()


def _feeder_run(f, compute, real, copy_ms, compute_ms, rep, prime=False):
    """One run of FEEDER_STEPS steps on `compute`; copy_ms: a hold on copy_stream before the first copy is issued; compute_ms: a hold
    on `compute` in front of every step's clones -> [(step, clip)] whose clone differs from the step's host clip."""
    snaps = []

    def fn(bufs):
        if compute_ms:
            hold(compute_ms)
            if not snaps:
                ev = torch.cuda.Event()
                ev.record()
                rep.vacuous |= not runs_beside(ev, f.copy_stream)
        snaps.append([snap(b) for b in bufs])

    with torch.cuda.stream(compute):
        if copy_ms:
            rep.vacuous |= not runs_beside(held_event(f.copy_stream, copy_ms), compute)
        if prime:
            f.prime()
        f.run(FEEDER_STEPS, fn)
    torch.cuda.synchronize()
    return [(k, j) for k in range(FEEDER_STEPS) for j in range(2) if not bits_equal(snaps[k][j].cpu(), real[2 * k + j])]


def _feeder(which):
    real, decoy = _feeder_inputs()
    f = feeder.PinnedClipFeeder(real, 2, device())
    compute = beside(f.copy_stream)
    rep = Report(tried=TRIED[-1])
    with torch.cuda.stream(compute):
        _, rep.host_ms = ms_of(lambda: f.run(FEEDER_STEPS, lambda bufs: [snap(b) for b in bufs]))      # the feeder's first run: warms it, and its host time (no less than a warm run's) sizes the hold
    torch.cuda.synchronize()
    _feeder_fill(f, decoy)
    rep.hold_ms = hold_for(rep.host_ms)
    if which == "ready":
        rep.mismatch = _feeder_run(f, compute, real, rep.hold_ms, 0, rep)
    elif which == "free":
        rep.mismatch = _feeder_run(f, compute, real, 0, rep.hold_ms, rep)
    else:                                   # a primed run, then a second run on the same feeder, both holds on
        first = _feeder_run(f, compute, real, rep.hold_ms, rep.hold_ms, rep, prime=True)
        second = _feeder_run(f, compute, real, rep.hold_ms, rep.hold_ms, rep)
        rep.mismatch = [("primed",) + m for m in first] + [("second",) + m for m in second]
    return rep


def feeder_copy_to_compute():
    """1: the copy stream is held before run(); every step's clones (on the compute stream) are that step's host clips: `ready`."""
    return _feeder("ready")


def feeder_compute_to_reuse():
    """2: every step's clones sit behind a hold on the compute stream; the copies of step k+2 go into step k's slot: `free`."""
    return _feeder("free")


def feeder_primed_and_second_run():
    """3: prime() + run(), then run() again on the same feeder (its slots hold the last run's clips), under both holds."""
    return _feeder("both")


# ---- ClipStager (scenarios 4 - 7) -------------------------------------------------------------------------------------------------------
def _batch(seed, which=REAL, shapes=FEEDER_SHAPES):
    return [torch.from_numpy(clip_bytes(s, seed * 10 + j, which)).pin_memory() for j, s in enumerate(shapes)]


def _stage(st, clips):
    st.begin(len(clips))
    devs = [st.add(c) for c in clips]
    return devs, st.end()


def _stager_with_decoys(compute):
    """A stager whose two slots hold decoy batches of the scenarios' shapes, staged and consumed on `compute` as the driver does"""
    st = compute["st"]
    with torch.cuda.stream(compute["s"]):
        for turn in range(2):
            devs, token = _stage(st, _batch(90 + turn, DECOY))
            st.wait(token)
            [snap(d) for d in devs]
            st.done_with(token)
            st.copies_landed(token)
    torch.cuda.synchronize()


def _new_stager():
    st = dataset.ClipStager(device())
    s = beside(st.copy_stream)
    return {"st": st, "s": s}, Report(tried=TRIED[-1])


def stager_copy_to_compute():
    """4: copy_stream is held, a batch is staged into a slot that holds another batch's bytes, wait(token), clones: `ready`."""
    env, rep = _new_stager()
    st, s = env["st"], env["s"]
    _, rep.host_ms = ms_of(lambda: _stager_with_decoys(env))
    _stager_with_decoys(env)
    rep.hold_ms = hold_for(rep.host_ms / 2)                       # (the timed phase staged and consumed two batches)
    real = _batch(1)
    with torch.cuda.stream(s):
        rep.vacuous = not runs_beside(held_event(st.copy_stream, rep.hold_ms), s)
        devs, token = _stage(st, real)
        st.wait(token)
        snaps = [snap(d) for d in devs]
        st.done_with(token)
    torch.cuda.synchronize()
    rep.mismatch = [j for j in range(2) if not bits_equal(snaps[j].cpu(), real[j])]
    return rep


def stager_compute_to_reuse():
    """5: batch b's clones sit behind a hold on the compute stream; b+1 and b+2 are staged as the driver stages them (b+2 takes b's
    slot, done_with(b) after stage(b+1)); b's clones are b's clips: `_free`."""
    env, rep = _new_stager()
    st, s = env["st"], env["s"]
    _, rep.host_ms = ms_of(lambda: _stager_with_decoys(env))
    rep.hold_ms = hold_for(rep.host_ms)
    real = [_batch(1 + b) for b in range(3)]
    snaps = []
    with torch.cuda.stream(s):
        staged = _stage(st, real[0])
        for b in range(3):
            devs, token = staged
            st.wait(token)
            if b == 0:
                ev = held_event(s, rep.hold_ms)
                rep.vacuous = not runs_beside(ev, st.copy_stream)
            snaps.append([snap(d) for d in devs])
            if b + 1 < 3:
                staged = _stage(st, real[b + 1])
            st.done_with(token)
            st.copies_landed(token)
            st.reap()
    torch.cuda.synchronize()
    rep.mismatch = [(b, j) for b in range(3) for j in range(2) if not bits_equal(snaps[b][j].cpu(), real[b][j])]
    return rep


def stager_pinned_staging():
    """6: add(c, pinned_buf) with copy_stream held: reap() keeps the buffer (in _landing, its bytes in the gate's books) while the
    copy has not landed, hands it back afterwards; junk written into the returned buffer does not reach the device clip."""
    env, rep = _new_stager()
    st, s = env["st"], env["s"]
    data = torch.from_numpy(clip_bytes(FEEDER_SHAPES[0], 7))

    def once(ms):
        off = []
        view, buf = st.alloc_pinned(data.shape)
        view.copy_(data)
        in_use = st.gate.in_use
        with torch.cuda.stream(s):
            ev = held_event(st.copy_stream, ms) if ms else None
            if ms:
                rep.vacuous = not runs_beside(ev, s)
            st.begin(1)
            d = st.add(view, buf)
            token = st.end()
            st.reap()
            if ms:
                rep.vacuous |= ev.query()
                if len(st._landing) != 1 or st._landing[0][1] is not buf:
                    off.append("handed back while the copy was held")
                if st.gate.in_use != in_use:
                    off.append(f"gate.in_use {in_use} -> {st.gate.in_use} while the copy was held")
            st.copies_landed(token)
            st.reap()
            if st._landing or st.gate.in_use != in_use - buf.numel() or not any(b is buf for b in st._pinned_free.get(buf.numel(), [])):
                off.append("not handed back after the copy had landed")
            buf.fill_(0xEE)
            st.wait(token)
            got = snap(d)
            st.done_with(token)
        torch.cuda.synchronize()
        return off + (["device clip"] if not bits_equal(got.cpu(), data) else [])

    warm, rep.host_ms = ms_of(lambda: once(0))
    rep.hold_ms = hold_for(rep.host_ms)
    rep.mismatch = warm + once(rep.hold_ms)
    return rep


def stager_slot_growth():
    """7: a ragged batch whose second clip does not fit the block: add() replaces it, the first clip stays in the old one.  Its clone
    sits behind a hold on the compute stream; the views are dropped and copy_stream fills new tensors of the old block's size.  The
    clone is the clip: the old block was recorded on the compute stream."""
    env, rep = _new_stager()
    st, s = env["st"], env["s"]
    small = torch.from_numpy(clip_bytes(RAGGED[4], 4)).pin_memory()
    large = torch.from_numpy(clip_bytes(RAGGED[5], 5)).pin_memory()
    rep.hold_ms = hold_for(0.0)                                # the held phase is two clones, a `del` and four fills: timed below
    with torch.cuda.stream(s):
        st.begin(2)
        d_small = st.add(small)
        old = st._slots[st._cur["slot"]]
        old_bytes, old_ptr = old.numel(), old.data_ptr()
        del old
        d_large = st.add(large)
        if st._slots[st._cur["slot"]].data_ptr() == old_ptr:
            rep.mismatch.append("the slot did not grow")
        token = st.end()
        st.wait(token)
        t0 = time.perf_counter()
        ev = held_event(s, rep.hold_ms)
        rep.vacuous = not runs_beside(ev, st.copy_stream)
        got_small, got_large = snap(d_small), snap(d_large)
        del d_small
        with torch.cuda.stream(st.copy_stream):
            junk = [torch.full((old_bytes,), 0xEE, dtype=torch.uint8, device=device()) for _ in range(4)]
        rep.vacuous |= ev.query()
        rep.host_ms = (time.perf_counter() - t0) * 1e3
        st.done_with(token)
    torch.cuda.synchronize()
    rep.reused = any(j.data_ptr() == old_ptr for j in junk)
    rep.mismatch += _off(got_small, small, "small clip") + _off(got_large, large, "large clip")
    return rep


# ---- extract_dataset_clips under contention (scenarios 8 - 10) --------------------------------------------------------------------------
_passes = itertools.count(1)


def _sources(kind, tmp_path, consumer, salt=0):
    """-> (clips of the overlapped pass, clips of the inline twin)"""
    if kind == "host":
        return host_source(salt=salt), host_source(salt=salt)
    if kind == "alloc":
        return host_source(alloc=True, salt=salt), host_source(salt=salt)
    if kind == "png":
        d = tmp_path / "png"
        names = write_png_clips(d) if not d.exists() else [f"v{i}" for i in range(len(RAGGED))]
        return (sampling.GpuFrameLoader(str(d), names, device=device(), consumer_stream=consumer),
                lambda i: sampling.load_clip_from_frames(str(d), names[i]))
    if kind == "yuv":
        d = tmp_path / "yuv"
        paths, ws, hs = write_yuv_clips(d)
        return (sampling.GpuYuvLoader(paths, ws, hs, "yuv420p", 25, device=device(), consumer_stream=consumer),
                lambda i: sampling.load_clip_from_yuv(paths[i], ws[i], hs[i], "yuv420p", 25))
    raise ValueError(kind)


def dataset_pass(kind, heavy, tmp_path=None):
    """8 - 10: the overlapped pass (prefetch 2, 3 loader threads) of the ragged set on a stream beside the stager's copy stream, with
    the held stand-in engine, against the inline pass (prefetch 0) of the plain one.  heavy = "copy": the copy stream's holds are three
    times the compute stream's, so every batch's copies run late (a missing `ready` wait reads the slot before them); "compute": the
    other way round, so the reads run late (a missing `_free` wait, or a clip freed too early, is overwritten before them)."""
    dev = device()
    salt = next(_passes)        # other bytes in every pass of a session: what an earlier pass left in a recycled block is never this pass's clip
    _, twin = _sources(kind, tmp_path, None, salt)
    want, want_errors = run_pass(twin, FingerprintEngine(dev), prefetch=0)
    warm_clips, _ = _sources(kind, tmp_path, None)
    run_pass(warm_clips, FingerprintEngine(dev), prefetch=2, workers=3)                     # the loader threads' first calls
    _, ms = ms_of(lambda: run_pass(warm_clips, FingerprintEngine(dev), prefetch=2, workers=3))
    eng = FingerprintEngine(dev)
    stager = dataset._stager(eng)                                                          # a new one: its slots grow in this pass
    s = beside(stager.copy_stream, torch.cuda.default_stream(dev))           # (the loader threads call from the null stream)
    rep = Report(tried=TRIED[-1], host_ms=ms / (len(RAGGED) // 2))                         # one turn of the driver's loop
    light = hold_for(rep.host_ms)
    rep.hold_ms = hold_for(rep.host_ms, 3.0)
    eng.hold_ms, eng.copy_stream = ((light, rep.hold_ms) if heavy == "copy" else (rep.hold_ms, light)), stager.copy_stream
    clips, _ = _sources(kind, tmp_path, s, salt)
    grown, add = [], stager.add

    def spy(c, pinned_buf=None):
        st = stager._cur
        before, at = (stager._slots[st["slot"]], st["at"]) if st is not None and not c.is_cuda else (None, 0)
        d = add(c, pinned_buf)
        if at > 0 and stager._slots[st["slot"]] is not before:
            grown.append(at)
        return d

    stager.add = spy
    try:
        with torch.cuda.stream(s):
            rep.vacuous = not runs_beside(held_event(stager.copy_stream, SIDE_PROBE_MS), s)
            torch.cuda.synchronize()
            got, errors = run_pass(clips, eng, prefetch=2, workers=3)
    finally:
        del stager.add
    torch.cuda.synchronize()
    rep.vacuous |= bool(eng.vacuous) or eng.vacuous is None
    rep.grown, rep.errors = grown, errors
    rep.mismatch = [i for i in range(len(RAGGED)) if not bits_equal(got[i].cpu(), want[i].cpu())]
    if errors != want_errors:
        rep.mismatch.append(("errors", errors, want_errors))
    if [i for i, _ in want_errors] != [ERROR_CLIP, REFUSED_CLIP] or not torch.isfinite(want.cpu()[[i for i in range(len(RAGGED)) if i not in (ERROR_CLIP, REFUSED_CLIP)]]).all():
        rep.mismatch.append(("the inline pass", want_errors))
    if stager.gate.in_use != 0:
        rep.mismatch.append(("gate.in_use", stager.gate.in_use))
    if kind in ("host", "alloc") and not grown:
        rep.mismatch.append("no slot grew inside a batch")
    return rep


# ---- PngDecoder, GpuFrameLoader, GpuYuvLoader (scenarios 11 - 13) -----------------------------------------------------------------------
def _png_set(seed, which, hws):
    imgs = [clip_bytes(hw + (3,), seed + k, which) for k, hw in enumerate(hws)]
    return [png_bytes(a) for a in imgs], imgs


def decoder_inputs_behind_the_caller():
    """11: decode(out=view) while the caller's stream is held and, behind the hold, fills `out` with decoy bytes: the result is the
    decoded images (wait_stream(caller)), not the decoy."""
    dec = pngdecode.decoder_for(device())
    caller = beside(dec.stream)
    rep = Report(tried=TRIED[-1])
    srcs, imgs = _png_set(11, REAL, [PNG_HW] * 2)
    decoy = torch.from_numpy(np.stack([clip_bytes(PNG_HW + (3,), 12 + k, DECOY) for k in range(2)])).to(device())
    with torch.cuda.stream(caller):
        out = torch.empty_like(decoy)
        dec.decode(srcs, out=out)
        _, rep.host_ms = ms_of(lambda: dec.decode(srcs, out=out))
        rep.hold_ms = hold_for(rep.host_ms)
        caller.synchronize()
        ev = held_event(caller, rep.hold_ms)
        rep.vacuous = not runs_beside(ev, dec.stream)
        snap(decoy, out=out)
        got = dec.decode(srcs, out=out)
    torch.cuda.synchronize()
    rep.mismatch = _off(got, np.stack(imgs), "out")
    return rep


def _loader_cases(tmp_path):
    """-> {name: (owned stream, call(content 0 | 1, consumer) -> device result or list, twin(content) -> ndarray or list)} for scenarios
    12 and 13: two contents of one size per class."""
    dev = device()
    dec = pngdecode.decoder_for(dev)
    same = [_png_set(20 + 10 * v, REAL, [PNG_HW] * 2) for v in range(2)]
    ragged = [_png_set(40 + 10 * v, REAL, [PNG_HW, PNG_HW_OTHER]) for v in range(2)]
    dirs = [tmp_path / f"frames{v}" for v in range(2)]
    for v, d in enumerate(dirs):
        if not d.exists():
            d.mkdir(parents=True)
            c = clip_bytes((2, 2) + PNG_HW + (3,), 60 + v)
            for t in range(2):
                (d / f"vid_{12 * t}.png").write_bytes(png_bytes(c[t, 0]))
                (d / f"vid_{12 * t}_next.png").write_bytes(png_bytes(c[t, 1]))
    fb = sampling.yuv_frame_bytes(sampling.yuv_layout("yuv420p")[0], YUV_H, YUV_W)
    yuvs = [str(tmp_path / f"v{v}.yuv") for v in range(2)]
    for v, p in enumerate(yuvs):
        clip_bytes((26, fb), 70 + v).tofile(p)
    yuv = sampling.GpuYuvLoader(yuvs, YUV_W, YUV_H, "yuv420p", 25, device=dev)

    def frames(v, consumer):
        return sampling.GpuFrameLoader(str(dirs[v]), ["vid"], device=dev, consumer_stream=consumer)(0)

    def yuv_call(v, consumer):
        yuv.consumer = consumer if consumer is not None else torch.cuda.current_stream(dev)
        return yuv(v)

    return {
        "PngDecoder[same]": (dec.stream, lambda v, c: dec.decode(same[v][0], consumer=c), lambda v: np.stack(same[v][1])),
        "PngDecoder[sizes differ]": (dec.stream, lambda v, c: dec.decode(ragged[v][0], consumer=c), lambda v: ragged[v][1]),
        "GpuFrameLoader": (dec.stream, frames, lambda v: sampling.load_clip_from_frames(str(dirs[v]), "vid")),
        "GpuYuvLoader": (yuv._state().stream, yuv_call, lambda v: sampling.load_clip_from_yuv(yuvs[v], YUV_W, YUV_H, "yuv420p", 25)),
    }


LOADER_CASES = ["PngDecoder[same]", "PngDecoder[sizes differ]", "GpuFrameLoader", "GpuYuvLoader"]


def _parts(x):
    return list(x) if isinstance(x, (list, tuple)) else [x]


def _parts_off(snaps, want, tag):
    want = _parts(want)
    return [tag] if len(snaps) != len(want) or any(not bits_equal(s.cpu(), torch.as_tensor(w)) for s, w in zip(snaps, want)) else []


def complete_on_return(name, tmp_path):
    """12: the owned stream is held before the call; right after the return a clone on a stream that never waited for anything is the
    host twin's bytes: the call came back only after its stream had finished."""
    owned, call, twin = _loader_cases(tmp_path)[name]
    fresh = beside(owned)
    rep = Report(tried=TRIED[-1])
    call(1, None)
    _, rep.host_ms = ms_of(lambda: call(1, None))               # (dropped: content 1 lies in the pool's free block of this size)
    rep.hold_ms = hold_for(rep.host_ms)
    torch.cuda.synchronize()
    ev = held_event(owned, rep.hold_ms)
    rep.vacuous = not runs_beside(ev, fresh)
    res = call(0, None)
    with torch.cuda.stream(fresh):
        snaps = [snap(p) for p in _parts(res)]
    torch.cuda.synchronize()
    rep.mismatch = _parts_off(snaps, twin(0), "result")
    return rep


def lifetime_on_the_consumer(name, tmp_path):
    """13: a result taken for consumer c; c is held with a clone of the result behind the hold; the result is dropped and a second
    call of the same size and other content is made.  The second result is not the first's storage, and the clone is the first
    content: the result was recorded on c."""
    owned, call, twin = _loader_cases(tmp_path)[name]
    caller = torch.cuda.default_stream(device())                # the calls below are made from it
    c = beside(owned, caller)
    rep = Report(tried=TRIED[-1])
    warm = [call(1, None), call(1, None)]                       # two results alive at once: the pool of the owned stream holds two blocks
    del warm                                                    # of this size, and nothing asks the driver for memory inside the hold
    _, rep.host_ms = ms_of(lambda: call(1, None))
    rep.hold_ms = hold_for(rep.host_ms)
    torch.cuda.synchronize()
    first = call(0, c)
    ptr = min(p.data_ptr() for p in _parts(first))
    with torch.cuda.stream(c):
        snaps = [torch.empty_like(p) for p in _parts(first)]
    ev = held_event(c, rep.hold_ms)
    rep.vacuous = not (runs_beside(ev, owned) and runs_beside(ev, caller))
    with torch.cuda.stream(c):
        for s, p in zip(snaps, _parts(first)):
            snap(p, out=s)
    del first, p
    second, rep.second_ms = ms_of(lambda: call(1, c))
    rep.notes = f"probe beside the hold: {not rep.vacuous}, second call {rep.second_ms:.2f} ms, hold still on after it: {not ev.query()}"
    rep.vacuous |= ev.query()
    if min(p.data_ptr() for p in _parts(second)) == ptr:
        rep.mismatch.append("the second result lies in the first's storage")
    torch.cuda.synchronize()
    rep.mismatch += _parts_off(snaps, twin(0), "held clone") + _parts_off(_parts(second), twin(1), "second result")
    return rep


# ---- PngEncoder (scenario 14) -----------------------------------------------------------------------------------------------------------
ENCODER_CASES = ["contiguous", "strided", "host array"]


def encoder_images_behind_the_caller(layout):
    """14: the image holds decoy bytes and gets its content behind a hold on the caller's stream; the PNG that comes back decodes to
    the content.  strided: _prepare makes it contiguous on the caller's stream; host array: it is uploaded there."""
    enc = pngencode.encoder_for(device())
    caller = beside(enc.stream)
    rep = Report(tried=TRIED[-1])
    H, W = PNG_HW
    real, decoy = clip_bytes((H, W, 3), 80), clip_bytes((H, W, 3), 81, DECOY)
    with torch.cuda.stream(caller):
        if layout == "strided":
            store = torch.from_numpy(np.repeat(decoy, 2, axis=1)).to(device())
            img = store[:, ::2]
        else:
            img = torch.from_numpy(decoy).to(device())
        staged = torch.from_numpy(real).to(device())            # before the warm calls: the block their contiguous copy of a strided
        enc.encode([img])                                       # image leaves behind (decoy bytes) is the one the held call's copy gets
        _, rep.host_ms = ms_of(lambda: enc.encode([img]))
        rep.hold_ms = hold_for(rep.host_ms)
        caller.synchronize()
        ev = held_event(caller, rep.hold_ms)
        rep.vacuous = not runs_beside(ev, enc.stream)
        snap(staged, out=img)
        files = enc.encode([real if layout == "host array" else img])
    torch.cuda.synchronize()
    rep.mismatch = [] if np.array_equal(pngdecode._pillow_bgr(files[0]), real) else ["decoded PNG"]
    return rep
