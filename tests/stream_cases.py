"""The case table of the C-ABI stream contract (include/relax_hip.h: "`stream` is a hipStream_t passed as void* (0 = default stream).
All work is enqueued on it; no hidden synchronisation.").

One record per entry point of the header that takes a `relax_stream`, keyed by its C name ("name:variant" where one entry has two
behaviours worth holding, e.g. relax_optical_flow_flags with and without an initial flow).  tests/test_stream_contract_cpu.py holds the
table against the header; tests/test_gpu_stream_contract.py runs every record on a held side stream.  A new entry point declares
itself here: a Case in CASES, or a line in EXEMPT with the header sentence that backs it in EXEMPT_BACKING.

A record:
  kind        "enqueue": once warm the call only enqueues on the caller's stream; "waits": the header says the call waits for the stream
              or the device, or returns host data - `sentence` is the header's sentence that says so
  make(seed)  the device tensors the call reads, as a dict; REAL and DECOY give visibly different outputs
  call(eng, inputs)  -> tuple of output device tensors; through the RelaxEngine method where there is one, ctypes otherwise
  prepare(eng, inputs)  host-side state set-up that waits for the device by contract (relax_head_train_import); the runner calls it
              before every call, outside the held region and outside a capture
  precisions  PRECISIONS for anything that contracts under "gemm_precision", a shorter tuple where the entry refuses the others, None otherwise
  capture     the record also goes through capture and replay with changed input
  needs       weights / state the call needs on the shared engine ("rn50", "vit", "vgg16", "mlp", "trainer")

Importing this module needs no GPU; make / call / prepare do.
"""
import ctypes as C
import os
import zlib

import numpy as np
import torch

PRECISIONS = ("f16x2", "bf16x6", "fp32")
REAL, DECOY = 1, 2
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_train.npz")


class Case:
    def __init__(self, kind, make, call, precisions=None, capture=False, sentence=None, prepare=None, needs=()):
        assert kind in ("enqueue", "waits") and (sentence is not None) == (kind == "waits")
        self.kind, self.make, self.call, self.precisions, self.capture = kind, make, call, precisions, capture
        self.sentence, self.prepare, self.needs = sentence, prepare, tuple(needs)


def entry_of(key):
    """The C name of a table key ("relax_optical_flow_flags:initial" -> "relax_optical_flow_flags")."""
    return key.split(":")[0]


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------
_state = {}


def ensure(needs):
    """The shared engine with the weights / state `needs` names loaded (each once per module run)."""
    from relax_vqa_amd import synth
    from tests import gpu_common
    eng = gpu_common.engine()
    if "rn50" in needs:
        gpu_common.rn50_weights()
    if "vit" in needs:
        gpu_common.vit_weights("vit_base")
    if "vgg16" in needs and _state.get("vgg16") is not eng:
        eng.load_vgg16(synth.vgg16_state_dict())
        _state["vgg16"] = eng
    if "mlp" in needs and _state.get("mlp") is not eng:
        rng = np.random.RandomState(5)
        eng.load_mlp_head(synth.mlp_head_state_dict(256, 128, seed=23), rng.uniform(0.5, 2.0, 256), rng.uniform(-1, 1, 256),
                          rng.standard_normal(256))
        _state["mlp"] = eng
    if "trainer" in needs:
        _trainer(eng)
    return eng


def _rng(seed, salt):
    return np.random.RandomState(7919 * salt + seed)


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _f32(seed, salt, *shape, scale=1.0):
    return _cu((_rng(seed, salt).standard_normal(shape) * scale).astype(np.float32))


def _u8(seed, salt, *shape):
    return _cu(_rng(seed, salt).randint(0, 256, shape).astype(np.uint8))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _sp():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(eng, rc, what, handle=True):
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {eng.lib.relax_last_error(eng.h if handle else None).decode()}")


def _empty(shape, dtype):
    return torch.empty(shape, dtype=dtype, device="cuda")


def _host(values, dtype=torch.float64):
    """Host results of a "waits" entry as a device tensor, so the runner compares them like any other output."""
    return torch.as_tensor(np.ascontiguousarray(np.asarray(values, dtype=np.float64))).to("cuda", dtype)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
H, W = 96, 128             # clips: 2 pairs at 96 x 128 = 48 patches of 16 x 16, fewer than the 196 slots: the padding path runs too
FH, FW = 64, 96            # flow
T = 2


def _clip(seed, h=H, w=W):
    from relax_vqa_amd import synth
    return _cu(synth.synthetic_clip(T, h, w, clip_id=40 + seed))


def make_clip(seed):
    return {"clip": _clip(seed)}


def make_flow_clip(seed):
    return {"clip": _clip(seed, FH, FW)}


def make_flow_clip_init(seed):
    return {"clip": _clip(seed, FH, FW), "init": _f32(seed, 11, T, FH, FW, 2, scale=2.0)}


def make_images(seed):
    return {"images": _u8(seed, 12, T, H, W, 3)}


def make_positions(seed, slots=196):
    r = _rng(seed, 13)
    pos = np.stack([r.randint(-1, H // 16 + 1, (T, slots)), r.randint(-1, W // 16 + 1, (T, slots))], axis=2).astype(np.int32)
    return {"images": _u8(seed, 12, T, H, W, 3), "positions": _cu(pos), "counts": _cu(np.array([48, 30 + seed], np.int32))}


def make_overlay(seed):
    d = make_positions(seed)
    d["values"] = _cu(_rng(seed, 14).uniform(-0.1, 1.0, (T, 196)).astype(np.float32))
    d["lut"] = _u8(3, 15, 256, 3)       # the colour table is the same for both seeds
    return d


def make_two_frags(seed):
    return {"a": _u8(seed, 16, 2, 224, 224, 3), "b": _u8(seed, 17, 2, 224, 224, 3)}


def make_frags3(seed):
    return {"frags": _u8(seed, 18, 3, 224, 224, 3)}


def make_frags2(seed):
    return {"frags": _u8(seed, 18, 2, 224, 224, 3)}


def make_canvas(seed):
    return {"images": _u8(seed, 19, 2, 48, 80, 3)}       # 3 x 5 patches: 16 tokens, the streaming attention route


def make_resize_frames(seed):
    return {"frames": _u8(seed, 20, 2, 97, 131, 3)}


def make_flow_field(seed):
    return {"flow": _f32(seed, 21, T, FH, FW, 2, scale=3.0)}


YH, YW = 48, 64


def make_yuv8(seed):
    return {"planes": _u8(seed, 22, 2 * (YH * YW * 3 // 2))}


def make_yuv10(seed):
    return {"planes": _u8(seed, 23, 2 * (YH * YW * 3))}          # yuv420p10le: 2-byte samples, higher bits masked off


def _near_grey_yuv(seed, salt, depth):
    """Two 4:2:0 frames with chroma a few steps off neutral (by seed), so the records do not saturate: planes Y, U, V per frame."""
    r = _rng(seed, salt)
    one, dt = 1 << (depth - 8), (np.uint8 if depth == 8 else "<u2")
    frames = []
    for _ in range(2):
        y = r.randint(40 * one, 200 * one, YH * YW)
        uv = 128 * one + r.randint(-(2 + 3 * seed) * one, (3 + 3 * seed) * one, 2 * (YH // 2) * (YW // 2))
        frames.append(np.concatenate([y, uv]).astype(dt))
    return {"planes": _cu(np.concatenate(frames).view(np.uint8))}


def make_grey_yuv8(seed):
    return _near_grey_yuv(seed, 62, 8)


def make_grey_yuv10(seed):
    return _near_grey_yuv(seed, 63, 10)


def make_grey_frames(seed):
    r = _rng(seed, 24)
    g = r.randint(0, 256, (3, YH, YW, 1))
    return {"frames": _cu(np.clip(g + r.randint(-2 - seed, 3 + seed, (3, YH, YW, 3)), 0, 255).astype(np.uint8))}


def make_mlp(seed):
    return {"features": _f32(seed, 25, 5, 256)}


def make_metrics(seed):
    r = _rng(seed, 26)
    y = r.uniform(1, 5, 96)
    return {"y_true": _cu(y), "y_pred": _cu(60 + 8 * y + r.standard_normal(96) * (2 + seed))}


def make_bytes(seed):
    return {"src": _u8(seed, 27, 4096)}


def make_rows(seed):
    return {"rows": _f32(seed, 28, 5, 300)}


# ---- stage A ------------------------------------------------------------------------------------------------------------------------
def _pairs_args(clip):
    fb = clip.shape[2] * clip.shape[3] * 3
    return C.c_void_p(clip.data_ptr()), C.c_void_p(clip.data_ptr() + fb), 2 * fb


def call_fragment_pairs(eng, t):
    clip = t["clip"]
    pos, cnt = _empty((T, 196, 2), torch.int32), _empty((T,), torch.int32)
    ori, diff = _empty((T, 224, 224, 3), torch.uint8), _empty((T, 224, 224, 3), torch.uint8)
    o, n, stride = _pairs_args(clip)
    _ok(eng, eng.lib.relax_fragment_pairs(eng.h, o, n, stride, T, H, W, 196, _p(pos), _p(cnt), _p(ori), _p(diff), None, _sp()),
        "relax_fragment_pairs")
    return pos, cnt, ori, diff


def call_fragment_pairs_ex(eng, t):
    r = eng.fragment_pairs(t["clip"], patch_size=8, top_n=None, want_scores=True)
    return r["positions"], r["counts"], r["ori_frag"], r["diff_frag"], r["scores"]


def call_fragment_image(eng, t):
    pos, cnt, frag = _empty((T, 196, 2), torch.int32), _empty((T,), torch.int32), _empty((T, 224, 224, 3), torch.uint8)
    _ok(eng, eng.lib.relax_fragment_image(eng.h, _p(t["images"]), H * W * 3, T, H, W, 196, _p(pos), _p(cnt), _p(frag), None, _sp()),
        "relax_fragment_image")
    return pos, cnt, frag


def call_fragment_image_ex(eng, t):
    r = eng.fragment_image(t["images"], want_scores=True)
    return r["positions"], r["counts"], r["frag"], r["scores"]


def call_gather_patches(eng, t):
    frag = _empty((T, 224, 224, 3), torch.uint8)
    _ok(eng, eng.lib.relax_gather_patches(eng.h, _p(t["images"]), H * W * 3, T, H, W, _p(t["positions"]), _p(t["counts"]), _p(frag), _sp()),
        "relax_gather_patches")
    return (frag,)


def call_gather_patches_ex(eng, t):
    return (eng.gather_patches(t["images"], t["positions"], t["counts"]),)


def call_merge_fragments(eng, t):
    return (eng.merge_fragments(t["a"], t["b"]),)


def call_attention_overlay(eng, t):
    out = _empty((T, H, W, 3), torch.uint8)
    _ok(eng, eng.lib.relax_attention_overlay(eng.h, _p(t["images"]), H * W * 3, T, H, W, _p(t["positions"]), _p(t["counts"]), _p(t["values"]),
                                             _p(t["lut"]), _p(out), _sp()), "relax_attention_overlay")
    return (out,)


def call_attention_overlay_ex(eng, t):
    return (eng.attention_overlay(t["images"], t["positions"], t["counts"], t["values"], lut=t["lut"], patch_size=16),)


# ---- flow ---------------------------------------------------------------------------------------------------------------------------
def call_optical_flow(eng, t):
    return eng.optical_flow(t["clip"], want_flow=True, want_image=True)


def call_optical_flow_ex(eng, t):
    return eng.optical_flow_ex(t["clip"], want_flow=True, want_image=True, winsize=9, iterations=2)


def call_flow_gaussian(eng, t):
    return eng.optical_flow_flags(t["clip"], want_flow=True, want_image=True, flags=256)


def call_flow_initial(eng, t):
    return eng.optical_flow_flags(t["clip"], want_flow=True, want_image=True, flags=4, initial_flow=t["init"])


def call_flow_initial_level(eng, t):
    return (eng.flow_initial_level(t["init"]),)


def call_flow_to_rgb(eng, t):
    return (eng.flow_to_rgb(t["flow"]),)


# ---- resize -------------------------------------------------------------------------------------------------------------------------
def call_resize_frames(eng, t):
    return eng.resize_frames(t["frames"])


def call_resize_frames_ex(eng, t):
    return eng.resize_frames_to(t["frames"], (56, 72))


def call_resize_residual(eng, t):
    return eng.residual_resize(t["clip"], want_residual=True)


def call_resize_residual_ex(eng, t):
    return eng.residual_resize(t["clip"], want_residual=True, size=(56, 72))


# ---- backbones ----------------------------------------------------------------------------------------------------------------------
def call_resnet50(eng, t):
    return eng.resnet50_features(t["frags"])


def call_resnet50_clip(eng, t):
    return eng.resnet50_clip_features(t["frags"], 2)


def call_vgg16(eng, t):
    return eng.vgg16_features(t["frags"])


def call_vit_features(eng, t):
    n, dim = t["frags"].shape[0], eng.vit_dim
    tk, pl = _empty((n, 196, dim), torch.float32), _empty((n, 3 * dim), torch.float32)
    _ok(eng, eng.lib.relax_vit_features(eng.h, _p(t["frags"]), n, _p(tk), _p(pl), _sp()), "relax_vit_features")
    return tk, pl


def call_vit_features_ex(eng, t):
    n, dim = t["frags"].shape[0], eng.vit_dim
    tk, pl, at = _empty((n, 196, dim), torch.float32), _empty((n, 3 * dim), torch.float32), _empty((n, dim // 64, 197), torch.float32)
    _ok(eng, eng.lib.relax_vit_features_ex(eng.h, _p(t["frags"]), n, _p(tk), _p(pl), _p(at), _sp()), "relax_vit_features_ex")
    return tk, pl, at


def call_vit_canvas(eng, t):
    return eng.vit_features(t["images"], tokens=True, pooled=True, attention=True)


def call_vit_layers(eng, t):
    r = eng.vit_intermediate_layers(t["images"], n=2, tokens=True, cls=True, pooled=True)
    return r["tokens"], r["cls"], r["pooled"]


def call_mlp_head(eng, t):
    return (eng.mlp_head(t["features"]),)


# ---- composites: the clip passes the production drivers run under torch.cuda.stream(...) ---------------------------------------------
def call_clip_vectors(eng, t):
    return (eng.clip_vectors([t["clip"]]),)


def call_full_clip_vectors(eng, t):
    return (eng.full_clip_vectors([t["clip"]], flow=True),)


def call_whole_residual_vectors(eng, t):
    return (eng.whole_residual_vectors([t["clip"]]),)


def call_attention_overlays(eng, t):
    r = eng.attention_overlays(t["clip"], fragment="residual_merged_frag")
    return r["overlay"], r["attention"]


# ---- head training: the 200 x 128 golden of tests/test_gpu_head_train.py ------------------------------------------------------------
def _gold():
    if "gold" not in _state:
        g = np.load(GOLD)
        _state["gold"] = (g, {k[5:]: g[k] for k in g.files if k.startswith("init/")})
    return _state["gold"]


def _trainer(eng):
    from relax_vqa_amd import head_train
    tr = _state.get("trainer")
    if tr is None or tr.eng is not eng or getattr(eng, "_head_train_generation", None) != tr.generation:
        tr = _state["trainer"] = head_train.HeadTrainer(eng, 200, 128, max_batch=64)
    return tr


def prepare_trainer(eng, inputs):
    """relax_head_train_import waits for the device, so it runs before the hold: the golden's initial model goes into the snapshot set
    (2), a DECOY model into the live set (which also zeroes the momentum buffers, Adam's moments and its step count) and into the SWA
    set.  Every training call starts with relax_head_train_copy(live <- snapshot) on its own stream: a kernel that escaped onto
    another stream finds the decoy model."""
    from relax_vqa_amd import head_train
    tr = _trainer(eng)
    init = _gold()[1]
    decoy = {k: (np.asarray(v) * (0.5 if np.asarray(v).dtype.kind == "f" else 1)) for k, v in init.items()}
    tr.import_state(decoy, head_train.LIVE)
    tr.import_state(decoy, head_train.SWA)
    tr.import_state(init, head_train.BEST)


def make_train(seed):
    g, _ = _gold()
    eng = ensure(())
    x, y = np.asarray(g["x"]), np.asarray(g["y"])
    if seed == DECOY:
        x, y = np.ascontiguousarray(x[::-1]) * np.float32(0.75), np.ascontiguousarray(y[::-1])
    xp = eng.head_train_transform(_cu(x), _cu(np.ones(200)), _cu(np.zeros(200)))
    return {"xp": xp, "y": _cu(y), "index": _cu(np.asarray(g["batches"][seed - 1], np.int32)), "all": _cu(np.arange(48, dtype=np.int32))}


def make_train_raw(seed):
    g, _ = _gold()
    r = _rng(seed, 30)
    return {"x": _cu(np.asarray(g["x"]) * np.float32(seed)), "scale": _cu(r.uniform(0.5, 2.0, 200)), "min": _cu(r.uniform(-1, 1, 200))}


def make_criterion(seed):
    return {"pred": _f32(seed, 31, 48, scale=10.0), "target": _f32(seed, 32, 48, scale=10.0)}


def _restart(eng):
    from relax_vqa_amd import head_train
    tr = _trainer(eng)
    tr.copy(head_train.LIVE, head_train.BEST)
    return tr


def _sgd(tr, t):
    return tr.step(t["xp"], t["y"], t["index"], 0.05, 0.9, 0.005, 0.6, 1.0, 0.1, seed=9, step=0, want_masks=True)


def _adam(tr, t):
    return tr.step_adam(t["xp"], t["y"], t["index"], 1e-3, 0.9, 0.999, 1e-8, 0.005, False, 0.6, 1.0, 0.1, seed=9, step=0, want_masks=True)


def _preds(tr, t, which=0):
    return tr.evaluate(t["xp"], None, t["all"], which)


def call_fit_scaler(eng, t):
    out = _empty((5, 200), torch.float64)
    _ok(eng, eng.lib.relax_head_fit_scaler(eng.h, _p(t["x"]), 48, 200, *[_p(out[i]) for i in range(5)], _sp()), "relax_head_fit_scaler")
    return (out,)


def call_train_transform(eng, t):
    return (eng.head_train_transform(t["x"], t["scale"], t["min"]),)


def call_train_copy(eng, t):
    return (_preds(_restart(eng), t),)


def call_criterion(eng, t):
    return _trainer(eng).criterion(t["pred"], t["target"])


def call_train_step(eng, t):
    tr = _restart(eng)
    m1, m2 = _sgd(tr, t)
    return _preds(tr, t), m1, m2


def call_train_step_adam(eng, t):
    tr = _restart(eng)
    m1, m2 = _adam(tr, t)
    return _preds(tr, t), m1, m2


def call_train_eval(eng, t):
    return (_restart(eng).evaluate(t["xp"], t["y"], t["index"]),)


def call_train_bn_pass(eng, t):
    tr = _restart(eng)
    tr.bn_pass(t["xp"], t["index"], 0, reset=True)
    return (_preds(tr, t),)


def call_train_swa_update(eng, t):
    from relax_vqa_amd import head_train
    tr = _restart(eng)
    tr.copy(head_train.SWA, head_train.BEST)
    _sgd(tr, t)
    tr.swa_update()
    return (_preds(tr, t, head_train.SWA),)


def call_train_dw1(eng, t):
    tr = _restart(eng)
    _sgd(tr, t)
    tr.dw1_only(True, 16, 0.05, 0.9, 0.005)
    return (_preds(tr, t),)


def call_train_dw1_adam(eng, t):
    tr = _restart(eng)
    _adam(tr, t)
    tr.dw1_adam_only(True, 16, 1e-3)
    return (_preds(tr, t),)


def call_train_export(eng, t):
    tr = _restart(eng)
    _sgd(tr, t)
    sd = tr.export_state()
    return (_host(np.concatenate([np.asarray(sd[k], np.float64).reshape(-1) for k in sorted(sd)])),)


def call_train_export_optimizer(eng, t):
    tr = _restart(eng)
    _adam(tr, t)
    st = tr.export_optimizer_state()
    return (_host(np.concatenate([st[m][k].reshape(-1) for m in ("exp_avg", "exp_avg_sq") for k in sorted(st[m])] + [np.array([st["step"]])])),)


def call_train_loss_read(eng, t):
    tr = _restart(eng)
    tr.read_loss(0, reset=True)
    _sgd(tr, t)
    return (_host(tr.read_loss(0, reset=True)),)


def call_train_pad_abs_sum(eng, t):
    tr = _restart(eng)
    _sgd(tr, t)
    pads = _host(tr.pad_abs_sum())      # zero for every input: the predictions beside it tell the inputs apart
    return pads, _preds(tr, t)


def call_train_pad_abs_sum_adam(eng, t):
    tr = _restart(eng)
    _adam(tr, t)
    pads = _host(tr.pad_abs_sum_adam())
    return pads, _preds(tr, t)


# ---- metrics ------------------------------------------------------------------------------------------------------------------------
def call_metrics_correlation(eng, t):
    from relax_vqa_amd import metrics
    fitted = _empty((96,), torch.float64)
    return metrics.correlation_metrics_async(eng, t["y_true"], t["y_pred"], fitted=fitted), fitted


def call_metrics_correlation_host(eng, t):
    r = eng.correlation_metrics(t["y_true"], t["y_pred"], return_fitted=True)
    return _host([r["plcc"], r["rmse"], r["srcc"], r["krcc"], *r["popt"], r["cost"]]), r["y_pred_logistic"]


def call_metrics_kendall(eng, t):
    from relax_vqa_amd import metrics
    return (metrics.kendall_async(eng, t["y_true"], t["y_pred"]),)


def call_metrics_kendall_host(eng, t):
    r = eng.kendall(t["y_true"], t["y_pred"])
    return (_host([r["krcc"], r["srcc"], r["S"], r["n1"], r["n2"], r["n0"]]),)


def call_metrics_pair_counts(eng, t):
    counts = _empty((5, 96), torch.int32)
    _ok(eng, eng.lib.relax_metrics_pair_counts(eng.h, _p(t["y_true"]), _p(t["y_pred"]), 96, _p(counts), _sp()), "relax_metrics_pair_counts")
    return (counts,)


# ---- operators ----------------------------------------------------------------------------------------------------------------------
def make_gemm(seed):
    return {"A": _f32(seed, 40, 300, 256), "W": _f32(seed, 41, 256, 256, scale=0.06), "bias": _f32(seed, 42, 256)}


def call_op_gemm(eng, t):
    return (eng.op_gemm(t["A"], t["W"], t["bias"], None, act=2),)


def make_conv(seed):
    from relax_vqa_amd.engine import pack_conv_weight
    w = (_rng(seed, 43).standard_normal((64, 64, 3, 3)) * 0.04).astype(np.float32)
    return {"x": _f32(seed, 44, 2, 14, 14, 64), "w": _cu(pack_conv_weight(w)), "bias": _f32(seed, 45, 64, scale=0.1)}


def call_op_conv(eng, t):
    return (eng.op_conv2d_nhwc(t["x"], t["w"], t["bias"], None, 64, 3, 3, 1, 1, 1),)


def call_op_conv_ex(eng, t):
    r = eng.op_conv2d_nhwc_ex(t["x"], t["w"], t["bias"], 64, 3, 3, 1, 1, act=1, amax=True)
    return r["out"], r["amax"]


def make_layernorm(seed):
    return {"x": _f32(seed, 46, 5, 384), "g": _f32(seed, 47, 384), "b": _f32(seed, 48, 384)}


def call_op_layernorm(eng, t):
    return (eng.op_layernorm(t["x"], t["g"], t["b"], 1e-6),)


def make_qkv(seed):
    return {"qkv": _f32(seed, 49, 2 * 197, 3 * 3 * 64)}


def call_op_attention(eng, t):
    return (eng.op_attention(t["qkv"], 2, 3),)


def make_qkv65(seed):
    return {"qkv": _f32(seed, 50, 2 * 65, 3 * 3 * 64)}


def call_op_attention_ex(eng, t):
    return (eng.op_attention_ex(t["qkv"], 2, 65, 3),)


def make_maxpool(seed):
    return {"x": _f32(seed, 51, 2, 16, 16, 64), "scale": _f32(seed, 52, 64), "shift": _f32(seed, 53, 64)}


def call_op_maxpool(eng, t):
    return (eng.op_bn_relu_maxpool(t["x"], t["scale"], t["shift"]),)


def call_op_maxpool_amax(eng, t):
    amax = _empty((2,), torch.int32)
    return eng.op_bn_relu_maxpool(t["x"], t["scale"], t["shift"], amax_out=amax), amax


def make_gap(seed):
    return {"x": _f32(seed, 54, 2, 49, 256)}


def call_op_gap(eng, t):
    return (eng.op_gap(t["x"]),)


def make_pool_vectors(seed):
    return {"v": _f32(seed, 58, 2, 2048)}


def call_op_pool_stats(eng, t):
    return (eng.op_pool_stats(t["v"], 2048),)


def make_tokens(seed):
    return {"x": _f32(seed, 55, 2, 50, 384), "g": _f32(seed, 56, 384), "b": _f32(seed, 57, 384)}


def call_op_token_stats(eng, t):
    return (eng.op_token_stats(t["x"]),)


def call_op_vit_norm_token_stats(eng, t):
    return eng.op_vit_norm_token_stats(t["x"], t["g"], t["b"], 1e-6)


def call_copy_bytes(eng, t):
    dst = _empty((4096,), torch.uint8)
    _ok(eng, eng.lib.relax_copy_bytes(eng.h, _p(t["src"]), _p(dst), 4096, _sp()), "relax_copy_bytes")
    return (dst,)


def call_segment_mean(eng, t):
    return (eng.rows_mean(t["rows"]),)


# ---- PNG ----------------------------------------------------------------------------------------------------------------------------
PH, PW, PSLOT = 24, 20, 4096


def make_png_streams(seed):
    """Two RGB images as zlib streams in fixed slots of one byte buffer (the streams' lengths differ by seed; the slots do not)."""
    r = _rng(seed, 60)
    src, items = np.zeros(2 * PSLOT, np.uint8), np.zeros((2, 8), np.int64)
    for n in range(2):
        rows = np.zeros((PH, 1 + PW * 3), np.uint8)
        rows[:, 0] = r.randint(0, 5, PH)                                   # a row filter each
        rows[:, 1:] = r.randint(0, 24, (PH, PW * 3))                       # few symbols: dynamic Huffman blocks with matches
        z = np.frombuffer(zlib.compress(rows.tobytes(), 6), np.uint8)
        assert z.size <= PSLOT
        src[n * PSLOT:n * PSLOT + z.size] = z
        items[n] = (n * PSLOT, z.size, n * rows.size, n * PH * PW * 3, PH, PW, 3, 0)
    return {"src": _cu(src), "items": _cu(items)}


def call_png_decode(eng, t):
    out, raw, status = _empty((2 * PH * PW * 3,), torch.uint8), _empty((2 * PH * (1 + PW * 3),), torch.uint8), _empty((2,), torch.int32)
    _ok(eng, eng.lib.relax_png_decode(_p(t["src"]), t["src"].numel(), _p(t["items"]), 2, _p(out), out.numel(), _p(raw), raw.numel(),
                                      _p(status), _sp()), "relax_png_decode", handle=False)
    return out, status


def make_png_images(seed):
    r = _rng(seed, 61)
    return {"images": _cu((r.randint(0, 256, (2, PH, PW, 1)) + r.randint(0, 8, (2, PH, PW, 3))).clip(0, 255).astype(np.uint8))}


def _png_encode_layout(eng):
    if "png_layout" not in _state:
        scratch, rows = C.c_int64(0), C.c_int(0)
        cap = int(eng.lib.relax_png_encode_bound(PH, PW, 3, -1, C.byref(scratch), C.byref(rows)))
        assert cap > 0
        slot = (cap + 7) // 8 * 8
        items = np.array([(n * PH * PW * 3, PW * 3, PH, PW, 3, n * slot, cap, -1) for n in range(2)], np.int64)
        _state["png_layout"] = (_cu(items), 2 * slot, max(2 * int(scratch.value), 64 + 64 * 2))
    return _state["png_layout"]


def _png_encode(eng, t, passes):
    items, out_bytes, scratch_bytes = _png_encode_layout(eng)
    out = torch.zeros((out_bytes,), dtype=torch.uint8, device="cuda")       # bytes past a stream's length are not the call's
    scratch = _empty(((scratch_bytes + 7) // 8,), torch.int64)
    lengths, status = _empty((2,), torch.int64), _empty((2,), torch.int32)
    args = (_p(t["images"]), t["images"].numel(), _p(items), 2, _p(out), out_bytes, _p(scratch), scratch.numel() * 8, _p(lengths), _p(status))
    if passes is None:
        _ok(eng, eng.lib.relax_png_encode(*args, _sp()), "relax_png_encode", handle=False)
    else:
        _ok(eng, eng.lib.relax_png_encode_passes(*args, passes, _sp()), "relax_png_encode_passes", handle=False)
    return out, lengths, status


def call_png_encode(eng, t):
    return _png_encode(eng, t, None)


def call_png_encode_passes(eng, t):
    return _png_encode(eng, t, 15)


# ---- raw YUV and the greyscale screen -------------------------------------------------------------------------------------------------
def call_yuv_to_bgr(eng, t):
    return (eng.yuv_to_bgr(t["planes"], YH, YW, "yuv420p"),)


def call_yuv_to_bgr_ex(eng, t):
    return (eng.yuv_to_bgr_ex(t["planes"], YH, YW, "yuv420p10le"),)


def call_greyscale_scan(eng, t):
    return (eng.greyscale_scan(t["frames"])["records"],)


def call_yuv_greyscale_scan(eng, t):
    return (eng.yuv_greyscale_scan(t["planes"], YH, YW, "yuv420p")["records"],)


def call_yuv_greyscale_scan_ex(eng, t):
    return (eng.yuv_greyscale_scan_ex(t["planes"], YH, YW, "yuv420p10le")["records"],)


# ---- the table ----------------------------------------------------------------------------------------------------------------------
def _e(make, call, **kw):
    return Case("enqueue", make, call, **kw)


def _w(sentence, make, call, **kw):
    return Case("waits", make, call, sentence=sentence, **kw)


TR = dict(prepare=prepare_trainer, needs=("trainer",))
WAITS_STREAM = "Waits for `stream`."

CASES = {
    # stage A
    "relax_fragment_pairs": _e(make_clip, call_fragment_pairs),
    "relax_fragment_pairs_ex": _e(make_clip, call_fragment_pairs_ex, capture=True),
    "relax_fragment_image": _e(make_images, call_fragment_image),
    "relax_fragment_image_ex": _e(make_images, call_fragment_image_ex),
    "relax_gather_patches": _e(make_positions, call_gather_patches),
    "relax_gather_patches_ex": _e(make_positions, call_gather_patches_ex),
    "relax_merge_fragments": _e(make_two_frags, call_merge_fragments),
    "relax_attention_overlay": _e(make_overlay, call_attention_overlay),
    "relax_attention_overlay_ex": _e(make_overlay, call_attention_overlay_ex, needs=("vit",)),
    # flow
    "relax_optical_flow": _e(make_flow_clip, call_optical_flow),
    "relax_optical_flow_ex": _e(make_flow_clip, call_optical_flow_ex),
    "relax_optical_flow_flags": _e(make_flow_clip, call_flow_gaussian),
    "relax_optical_flow_flags:initial_flow": _w("The call waits for the stream once per chunk (the host tables of the resize).",
                                                make_flow_clip_init, call_flow_initial),
    "relax_flow_initial_level": _w("Waits for the stream.", make_flow_clip_init, call_flow_initial_level),
    "relax_flow_to_rgb": _e(make_flow_field, call_flow_to_rgb),
    # resize
    "relax_resize_frames": _e(make_resize_frames, call_resize_frames),
    "relax_resize_residual": _e(make_clip, call_resize_residual),
    "relax_resize_frames_ex": _e(make_resize_frames, call_resize_frames_ex, capture=True),
    "relax_resize_residual_ex": _e(make_clip, call_resize_residual_ex),
    # backbones and the inference head
    "relax_resnet50_features": _e(make_frags3, call_resnet50, precisions=PRECISIONS, needs=("rn50",)),
    "relax_resnet50_clip_features": _e(make_frags3, call_resnet50_clip, precisions=PRECISIONS, needs=("rn50",)),
    "relax_vgg16_features": _e(make_frags2, call_vgg16, precisions=PRECISIONS, capture=True, needs=("vgg16",)),
    "relax_vit_features": _e(make_frags3, call_vit_features, precisions=PRECISIONS, needs=("vit",)),
    "relax_vit_features_ex": _e(make_frags3, call_vit_features_ex, precisions=PRECISIONS, needs=("vit",)),
    "relax_vit_features_canvas": _e(make_canvas, call_vit_canvas, precisions=PRECISIONS, capture=True, needs=("vit",)),
    "relax_vit_intermediate_layers": _e(make_canvas, call_vit_layers, precisions=PRECISIONS, capture=True, needs=("vit",)),
    "relax_mlp_head": _e(make_mlp, call_mlp_head, capture=True, needs=("mlp",)),
    # head training
    "relax_head_fit_scaler": _e(make_train_raw, call_fit_scaler),
    "relax_head_train_transform": _e(make_train_raw, call_train_transform),
    "relax_head_train_copy": _e(make_train, call_train_copy, **TR),
    "relax_head_criterion": _e(make_criterion, call_criterion, needs=("trainer",)),
    "relax_head_train_step": _e(make_train, call_train_step, **TR),
    "relax_head_train_step_adam": _e(make_train, call_train_step_adam, capture=True, **TR),
    "relax_head_train_eval": _e(make_train, call_train_eval, **TR),
    "relax_head_train_bn_pass": _e(make_train, call_train_bn_pass, **TR),
    "relax_head_train_swa_update": _e(make_train, call_train_swa_update, **TR),
    "relax_head_train_dw1": _e(make_train, call_train_dw1, **TR),
    "relax_head_train_dw1_adam": _e(make_train, call_train_dw1_adam, **TR),
    "relax_head_train_export": _w(WAITS_STREAM, make_train, call_train_export, **TR),
    "relax_head_train_export_optimizer": _w(WAITS_STREAM, make_train, call_train_export_optimizer, **TR),
    "relax_head_train_loss_read": _w("Waits for `stream`: the one read of an epoch.", make_train, call_train_loss_read, **TR),
    "relax_head_train_pad_abs_sum": _w(WAITS_STREAM, make_train, call_train_pad_abs_sum, **TR),
    "relax_head_train_pad_abs_sum_adam": _w("Waits for `stream`, as relax_head_train_pad_abs_sum does.", make_train,
                                            call_train_pad_abs_sum_adam, **TR),
    # metrics
    "relax_metrics_correlation": _e(make_metrics, call_metrics_correlation),
    "relax_metrics_correlation:host_out": _w("with `out` in host memory it copies the results and waits for `stream`.", make_metrics,
                                             call_metrics_correlation_host),
    "relax_metrics_kendall": _e(make_metrics, call_metrics_kendall),
    "relax_metrics_kendall:host_out": _w("out: 8 doubles, DEVICE or HOST (as above)", make_metrics, call_metrics_kendall_host),
    "relax_metrics_pair_counts": _e(make_metrics, call_metrics_pair_counts),
    # operators
    "relax_op_gemm": _e(make_gemm, call_op_gemm, precisions=PRECISIONS),
    "relax_op_conv2d_nhwc": _e(make_conv, call_op_conv, precisions=PRECISIONS),
    "relax_op_conv2d_nhwc_ex": _e(make_conv, call_op_conv_ex, precisions=("f16x2",)),     # (the entry refuses every other precision)
    "relax_op_layernorm": _e(make_layernorm, call_op_layernorm),
    "relax_op_attention": _e(make_qkv, call_op_attention, precisions=PRECISIONS),
    "relax_op_attention_ex": _e(make_qkv65, call_op_attention_ex, precisions=PRECISIONS),
    "relax_op_bn_relu_maxpool": _e(make_maxpool, call_op_maxpool),
    "relax_op_bn_relu_maxpool_amax": _e(make_maxpool, call_op_maxpool_amax),
    "relax_op_gap": _e(make_gap, call_op_gap),
    "relax_op_pool_stats": _e(make_pool_vectors, call_op_pool_stats),
    "relax_op_token_stats": _e(make_tokens, call_op_token_stats),
    "relax_op_vit_norm_token_stats": _e(make_tokens, call_op_vit_norm_token_stats),
    "relax_copy_bytes": _e(make_bytes, call_copy_bytes),
    "relax_segment_mean": _e(make_rows, call_segment_mean),
    # PNG, raw YUV, greyscale
    "relax_png_decode": _e(make_png_streams, call_png_decode),
    "relax_png_encode": _e(make_png_images, call_png_encode),
    "relax_png_encode_passes": _e(make_png_images, call_png_encode_passes),
    "relax_yuv_to_bgr": _e(make_yuv8, call_yuv_to_bgr),
    "relax_yuv_to_bgr_ex": _e(make_yuv10, call_yuv_to_bgr_ex, capture=True),
    "relax_greyscale_scan": _e(make_grey_frames, call_greyscale_scan),
    "relax_yuv_greyscale_scan": _e(make_grey_yuv8, call_yuv_greyscale_scan),
    "relax_yuv_greyscale_scan_ex": _e(make_grey_yuv10, call_yuv_greyscale_scan_ex),
}

# RelaxEngine methods that chain several entries: what dataset.py / feeder.py run on their side streams.  Same record, no C name.
COMPOSITES = {
    "clip_vectors": _e(make_clip, call_clip_vectors, precisions=PRECISIONS, capture=True, needs=("rn50", "vit")),
    "full_clip_vectors(flow=True)": _e(make_clip, call_full_clip_vectors, precisions=PRECISIONS, capture=True, needs=("rn50", "vit")),
    "whole_residual_vectors": _e(make_clip, call_whole_residual_vectors, capture=True, needs=("rn50", "vit")),
    "attention_overlays": _e(make_clip, call_attention_overlays, needs=("vit",)),
}

# Entries with a relax_stream that cannot be staged: {C name: reason}; EXEMPT_BACKING has the header sentence behind each.
EXEMPT = {
    "relax_vit_pos_embed": "reads nothing but the loaded weights, so a real and a decoy input cannot differ; its cached-table path is "
                           "held through relax_vit_features_canvas and relax_vit_intermediate_layers, which get their table from it",
}
EXEMPT_BACKING = {
    "relax_vit_pos_embed": "The same holds for relax_vit_features_canvas, which gets its table here.",
}
