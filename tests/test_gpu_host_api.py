"""The reference-named host API (relax-vqa_amd/extractor/*, main_fragment_layerstack) driven the way the
reference's own drivers drive it (PNG paths, per-frame lists), checked against the oracle."""
import os

import numpy as np
import pytest
from PIL import Image

import relax_vqa_amd  # noqa: F401
from oracle import fragment_ref, pooling_ref, resnet50_ref, vit_ref
from tests.gpu_common import assert_close, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from relax_vqa_amd import main_fragment_layerstack as m
    from relax_vqa_amd import runtime
    rn, vit = synth.resnet50_state_dict(), synth.vit_state_dict("vit_base")
    runtime.set_weights(resnet50=rn, vit=vit, vit_name="vit_base")
    return m, rn, vit


def _write_png_bgr(path, bgr):
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(path)   # cv2.imwrite stores BGR arrays as RGB PNGs


def test_driver_loop_like_the_reference(api, tmp_path):
    m, rn, vit = api
    T = 2
    clip = synth.synthetic_clip(T, 272, 400, clip_id=8)
    ori_acts, res_acts, vit_acts = [], [], []
    refs = []
    for t in range(T):
        img_original, img_next = clip[t, 0], clip[t, 1]
        # residual = cv2.absdiff(...); process_patches('frame_diff'); get_original_frame_patches  (fused on the GPU)
        diff_frag, ori_frag, positions = m.fragment_pair(img_original, img_next)
        ref = fragment_ref.fragment_pair(img_original, img_next)
        refs.append(ref)
        assert positions == [tuple(p) for p in ref["positions"].tolist()]
        assert np.array_equal(diff_frag, ref["diff_frag"]) and np.array_equal(ori_frag, ref["ori_frag"])
        # the step-by-step functions give the same answers
        residual = fragment_ref.absdiff(img_next, img_original)
        assert np.array_equal(m.get_patch_diff(residual, 16), ref["score"])
        path, frag2, pos2 = m.process_patches(str(tmp_path / f"v_{t}.png"), "frame_diff", residual, 16, 224, 196)
        assert path.endswith(f"v_{t}_residual_imp.png") and pos2 == positions and np.array_equal(frag2, diff_frag)
        assert np.array_equal(m.get_original_frame_patches(img_original, positions, 16, 224), ori_frag)
        # PNG round trip as the reference does it, then get_deep_feature on the paths
        ori_path = str(tmp_path / f"v_{t}_ori_frag.png")
        res_path = str(tmp_path / f"v_{t}_residual_imp.png")
        _write_png_bgr(ori_path, ori_frag)
        _write_png_bgr(res_path, diff_frag)
        _, _, a = m.get_deep_feature("resnet50", "v", ori_path, "original", "layer_stack")
        _, _, b = m.get_deep_feature("resnet50", "v", res_path, "original", "pool")
        _, _, c = m.get_deep_feature("vit", "v", ori_path, "original", "pool")
        assert list(a.keys()) == pooling_ref.RESNET50_TAPS and a["resnet50.conv1"].shape == (64, 112, 112)
        assert b.shape == (2048, 1, 1) and c.shape == (196, 768)
        ori_acts.append(a)
        res_acts.append(b)
        vit_acts.append(c)
    f_ori = m.process_video_feature(ori_acts, "resnet50", "layer_stack")
    f_res = m.process_video_feature(res_acts, "resnet50", "pool")
    f_vit = m.process_video_feature(vit_acts, "vit")
    combined = m.concatenate_features(f_ori, f_res)
    assert combined.shape == (T, 15171) and f_vit.shape == (T, 2304)
    tr = resnet50_ref.to_torch_state_dict(rn)
    ori = np.stack([r["ori_frag"] for r in refs])
    res = np.stack([r["diff_frag"] for r in refs])
    assert_close(f_ori, resnet50_ref.layer_stack_features(tr, ori), "driver layer_stack")
    assert_close(f_res, resnet50_ref.pool_features(tr, res), "driver pool")
    assert_close(f_vit, vit_ref.pool_features(vit_ref.to_torch_state_dict(vit), ori, 12), "driver vit pool")
    # raw dicts (no .pooled) are reduced on the GPU too
    plain = [dict(a) for a in ori_acts]
    assert_close(m.process_video_feature(plain, "resnet50", "layer_stack"), f_ori, "layer_stack from raw taps", rtol=1e-5)


def test_merge_and_flow_fragment_path(api):
    m, _, _ = api
    g = np.random.default_rng(3)
    flow_img = g.integers(0, 256, (272, 400, 3), dtype=np.uint8)
    _, frag, pos = m.process_patches("x_1.png", "optical_flow", flow_img, 16, 224, 196)
    want, wpos = fragment_ref.extract_important_patches(flow_img, fragment_ref.get_patch_diff(flow_img))
    assert np.array_equal(frag, want) and pos == [tuple(p) for p in wpos.tolist()]
    other = g.integers(0, 256, (224, 224, 3), dtype=np.uint8)
    assert np.array_equal(m.merge_fragments(frag, other), fragment_ref.merge_fragments(frag, other))


def test_unbuilt_rows_fail_loudly(api, tmp_path):
    m, _, _ = api
    assert m.flow_to_rgb(np.zeros((32, 32, 2), np.float32)).shape == (32, 32, 3)
    with pytest.raises(NotImplementedError):
        m.get_deep_feature("vgg16", "v", np.zeros((224, 224, 3), np.uint8), "original", "pool")


def test_whole_frame_path_like_main_layer_stack(api, tmp_path):
    """Whole sampled frames (src/main_layer_stack.py:81-151, src/demo_test.py:81-87): PIL-exact resize on the GPU, then
    the same backbones; checked against PIL + oracle."""
    m, rn, vit = api
    g = np.random.default_rng(17)
    frame = g.integers(0, 256, (270, 480, 3), dtype=np.uint8)          # BGR as cv2 holds it
    p = str(tmp_path / "vid_3.png")
    _write_png_bgr(p, frame)
    _, _, a = m.get_deep_feature("resnet50", "vid", p, "original", "layer_stack")
    _, _, c = m.get_deep_feature("vit", "vid", p, "original", "pool")
    pil = Image.open(p)
    rn_in = np.ascontiguousarray(np.asarray(pil.resize((224, 224), Image.BILINEAR))[..., ::-1])[None]
    vit_in = np.ascontiguousarray(np.asarray(pil.resize((224, 224), Image.LANCZOS))[..., ::-1])[None]
    want_ls = resnet50_ref.layer_stack_features(resnet50_ref.to_torch_state_dict(rn), rn_in)
    assert_close(m.process_video_feature([a], "resnet50", "layer_stack"), want_ls, "whole-frame layer_stack")
    want_tok = vit_ref.tokens(vit_ref.to_torch_state_dict(vit), vit_in, 12)[0]
    assert_close(c, want_tok, "whole-frame vit tokens")


def test_full_35203_vector(api):
    from relax_vqa_amd import runtime
    import torch
    m, rn, vit = api
    clip = synth.synthetic_clip(2, 272, 400, clip_id=12)
    vec = runtime.get_engine().full_clip_vector(torch.from_numpy(clip).cuda()).cpu().numpy()
    assert vec.shape == (35203,) and np.isfinite(vec).all()
    # whole-frame block against PIL + oracle
    from oracle import resize_ref
    rn_in = np.stack([resize_ref.resize(clip[t, 0], 224, 224, resize_ref.BILINEAR) for t in range(2)])
    want = resnet50_ref.layer_stack_features(resnet50_ref.to_torch_state_dict(rn), rn_in).mean(axis=0)
    assert_close(vec[:13120], want, "full vector: whole-frame ResNet block")


def test_batched_full_vectors_match_single(api):
    from relax_vqa_amd import runtime
    import torch
    eng = runtime.get_engine()
    a = torch.from_numpy(synth.synthetic_clip(2, 272, 400, clip_id=13)).cuda()
    b = torch.from_numpy(synth.synthetic_clip(1, 240, 320, clip_id=14)).cuda()
    both = eng.full_clip_vectors([a, b], flow=True)
    alone = torch.stack([eng.full_clip_vector(a, flow=True), eng.full_clip_vector(b, flow=True)])
    assert both.shape == (2, 35203)
    assert_close(both, alone.cpu().numpy(), "batched vs single full vectors", rtol=1e-4, atol_frac=1e-5)


def test_variant_drivers_keep_their_own_signatures(api, tmp_path):
    """main_residual_fragment / main_fragment_pool / main_layer_stack: the arities and layer names of those reference
    files (src/main_residual_fragment.py:83-214, src/main_fragment_pool.py:83-143, src/main_layer_stack.py:81-151)."""
    from relax_vqa_amd import main_fragment_pool as mp
    from relax_vqa_amd import main_layer_stack as ml
    from relax_vqa_amd import main_residual_fragment as mr
    m, rn, vit = api
    o, nx = synth.synthetic_pair(272, 400, 31)
    ref = fragment_ref.fragment_pair(o, nx)
    residual = fragment_ref.absdiff(nx, o)
    # residual-fragment driver: image only / path only; the fragment travels under its path name, not through a PNG
    assert np.array_equal(mr.extract_important_patches(residual, mr.get_patch_diff(residual, 16)), ref["diff_frag"])
    path = mr.process_patches(str(tmp_path / "a_1.png"), "frame_diff", residual, 16, 224, 196)
    assert isinstance(path, str) and path.endswith("a_1_residual_imp.png") and not os.path.exists(path)
    _, _, act = mr.get_deep_feature("resnet50", "a", path, "original", "pool")
    _, _, last = mr.get_deep_feature("resnet50", "a", ref["diff_frag"], "original", "last_layer")
    _, _, tok = mr.get_deep_feature("vit", "a", ref["diff_frag"], "original", "pool")
    assert act.shape == (2048, 1, 1) and last.shape == (2048, 7, 7) and tok.shape == (196, 768)
    tr = resnet50_ref.to_torch_state_dict(rn)
    assert_close(mr.process_video_feature([act], "resnet50"), resnet50_ref.pool_features(tr, ref["diff_frag"][None]),
                 "residual-fragment driver pool")
    assert_close(last.mean(axis=(1, 2)), np.asarray(act).reshape(-1), "last_layer tap vs avgpool")
    assert_close(mp.process_video_feature([tok], "vit"),
                 vit_ref.pool_features(vit_ref.to_torch_state_dict(vit), ref["diff_frag"][None], 12), "pool driver vit")
    with pytest.raises(NotImplementedError):
        mr.process_video_feature([last], "resnet50")
    with pytest.raises(ValueError):
        mr.get_deep_feature("resnet50", "a", ref["diff_frag"], "original", "layer_stack")
    # the pool driver returns triples like main_fragment_layerstack
    p2, frag2, pos2 = mp.process_patches(str(tmp_path / "a_1.png"), "optical_flow", residual, 16, 224, 196)
    assert p2.endswith("a_1_residual_of_imp.png") and np.array_equal(frag2, ref["diff_frag"])
    assert pos2 == [tuple(p) for p in ref["positions"].tolist()]
    # whole-frame driver: four / two arguments
    _, _, taps = ml.get_deep_feature("resnet50", "a", o, "original")
    rn_in = np.ascontiguousarray(np.asarray(Image.fromarray(np.ascontiguousarray(o[..., ::-1]))
                                            .resize((224, 224), Image.BILINEAR))[..., ::-1])[None]
    assert_close(ml.process_video_feature([taps], "resnet50"), resnet50_ref.layer_stack_features(tr, rn_in),
                 "whole-frame driver")
    _, _, wtok = ml.get_deep_feature("vit", "a", o, "original")
    assert ml.process_video_feature([wtok], "vit").shape == (1, 2304)
    with pytest.raises(NotImplementedError):
        ml.get_deep_feature("vgg16", "a", o, "original")


def test_full_35203_vector_every_block_against_the_oracle(api):
    """The whole demo_test vector, block by block: whole-frame ResNet-50 layer stack | whole-frame ViT stats | fragment
    layer stack | residual-fragment pool | ViT stats of the original and of the residual fragment (src/demo_test.py:89-175).
    The flow images come from the GPU and are handed to both sides, so the comparison does not hinge on a near-tie between
    two flow patches."""
    import torch
    from oracle import resize_ref
    from relax_vqa_amd import runtime
    m, rn, vit = api
    eng = runtime.get_engine()
    clip = synth.synthetic_clip(2, 272, 400, clip_id=21)
    frames = torch.from_numpy(clip).cuda()
    _, flow_img = eng.optical_flow(frames)
    vec = eng.full_clip_vector(frames, flow_images=flow_img).cpu().numpy()
    fimg = flow_img.cpu().numpy()
    tr, tv = resnet50_ref.to_torch_state_dict(rn), vit_ref.to_torch_state_dict(vit)
    ori, res, bil, lan = [], [], [], []
    for t in range(2):
        fp = fragment_ref.fragment_pair(clip[t, 0], clip[t, 1])
        flow_frag, _ = fragment_ref.extract_important_patches(fimg[t], fragment_ref.get_patch_diff(fimg[t]))
        ori.append(fp["ori_frag"])
        res.append(fragment_ref.merge_fragments(fp["diff_frag"], flow_frag))
        bil.append(resize_ref.resize(clip[t, 0], 224, 224, resize_ref.BILINEAR))
        lan.append(resize_ref.resize(clip[t, 0], 224, 224, resize_ref.LANCZOS))
    ori, res, bil, lan = (np.stack(a) for a in (ori, res, bil, lan))
    want = np.concatenate([
        resnet50_ref.layer_stack_features(tr, bil).mean(axis=0),
        vit_ref.pool_features(tv, lan, 12).mean(axis=0),
        resnet50_ref.layer_stack_features(tr, ori).mean(axis=0),
        resnet50_ref.pool_features(tr, res).mean(axis=0),
        vit_ref.pool_features(tv, ori, 12).mean(axis=0),
        vit_ref.pool_features(tv, res, 12).mean(axis=0)])
    assert want.shape == (35203,)
    edges = [0, 13120, 15424, 28544, 30595, 32899, 35203]
    names = ["whole-frame RN50 LS", "whole-frame ViT", "fragment RN50 LS", "residual RN50 pool", "ViT original frag", "ViT residual frag"]
    for a, b, nm in zip(edges[:-1], edges[1:], names):
        assert_close(vec[a:b], want[a:b], f"full vector block: {nm}")


def test_integration_md_ctypes_stub_runs_as_written(api):
    """INTEGRATION.md section 3 shows the binding a reference maintainer would add; run that very text (only the library path is
    made absolute) and compare with the engine."""
    import re
    import torch
    from relax_vqa_amd import _lib, runtime
    m, rn, vit = api
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    code = re.search(r"## 3\. Option B.*?```python\n(.*?)```", text, re.S).group(1)
    code = code.replace('C.CDLL("librelax_hip.so")', f'C.CDLL({_lib.LIB_PATH!r})')
    ns = {}
    exec(compile(code, "INTEGRATION.md", "exec"), ns)
    ns["load_resnet50"]({k: torch.from_numpy(np.asarray(v)) for k, v in rn.items()})
    frames = torch.from_numpy(synth.synthetic_clip(2, 240, 320, clip_id=44)).cuda()
    feats, pos = ns["fragment_and_features"](frames)
    torch.cuda.synchronize()
    want = runtime.get_engine().extract_clip(frames, vit=False)
    assert torch.equal(pos, want["positions"])
    assert_close(feats, want["resnet"].cpu().numpy(), "INTEGRATION.md stub vs engine", rtol=1e-5, atol_frac=1e-5)   # batch compositions differ


@pytest.mark.parametrize("form", ["plain", "state_dict_wrapper", "module_prefix"])
def test_checkpoint_files_go_through_the_loader_bit_for_bit(api, tmp_path, monkeypatch, form):
    """No test had pushed a FILE through runtime._load_file (round-2 review): torch.save the synthetic state dicts the way a
    user would hold torchvision / DINO checkpoints - plain, wrapped in {"state_dict": ...}, or with DataParallel's `module.`
    prefix - point RELAX_RESNET50_WEIGHTS / RELAX_VIT_WEIGHTS at them, and the reference-named API (get_deep_feature) must give
    the bits it gives with the same weights injected in memory (src/extractor/visualise_resnet.py:21,
    src/extractor/visualise_vit_layer.py:304-329)."""
    import torch
    from relax_vqa_amd import runtime
    m, rn, vit = api
    frag = fragment_ref.fragment_pair(*synth.synthetic_pair(240, 320, 71))["ori_frag"]
    eng = runtime.get_engine()
    eng.set_option("gemm_split_k", 0)
    try:
        runtime.set_weights(resnet50=rn, vit=vit, vit_name="vit_base")
        _, _, a0 = m.get_deep_feature("resnet50", "v", frag, "original", "layer_stack")
        _, _, b0 = m.get_deep_feature("resnet50", "v", frag, "original", "pool")
        _, _, c0 = m.get_deep_feature("vit", "v", frag, "original", "pool")

        def save(sd, name):
            t = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
            t["bn1.num_batches_tracked" if "conv1.weight" in sd else "extra.counter"] = torch.tensor(7)   # non-float entries are skipped
            if form == "module_prefix":
                t = {"module." + k: v for k, v in t.items()}
            if form == "state_dict_wrapper":
                t = {"state_dict": t, "epoch": 3}
            path = str(tmp_path / name)
            torch.save(t, path)
            return path

        monkeypatch.setenv("RELAX_RESNET50_WEIGHTS", save(rn, "resnet50.pth"))
        monkeypatch.setenv("RELAX_VIT_WEIGHTS", save(vit, "dino_vitbase16.pth"))
        monkeypatch.delenv("RELAX_ALLOW_SYNTHETIC_WEIGHTS", raising=False)
        # load something else first, so that the file load provably replaces what the engine holds
        runtime.set_weights(resnet50=synth.resnet50_state_dict(adversarial=True), vit=synth.vit_state_dict("vit_base", adversarial=True))
        runtime.reset_weights()
        _, _, a1 = m.get_deep_feature("resnet50", "v", frag, "original", "layer_stack")
        _, _, b1 = m.get_deep_feature("resnet50", "v", frag, "original", "pool")
        _, _, c1 = m.get_deep_feature("vit", "v", frag, "original", "pool")
        assert list(a1.keys()) == list(a0.keys())
        for k in a0:
            assert np.array_equal(a0[k], a1[k]), k
        assert np.array_equal(a0.pooled, a1.pooled) and np.array_equal(b0, b1) and np.array_equal(b0.pooled, b1.pooled)
        assert np.array_equal(c0, c1)
        # a missing file / a missing variable are errors, not a silent fall-back to synthetic weights
        monkeypatch.setenv("RELAX_RESNET50_WEIGHTS", str(tmp_path / "nope.pth"))
        runtime.reset_weights()
        with pytest.raises((OSError, RuntimeError)):
            m.get_deep_feature("resnet50", "v", frag, "original", "pool")
        monkeypatch.delenv("RELAX_RESNET50_WEIGHTS")
        with pytest.raises(RuntimeError, match="RELAX_RESNET50_WEIGHTS is not set"):
            m.get_deep_feature("resnet50", "v", frag, "original", "pool")
    finally:
        eng.set_option("gemm_split_k", 1)
        runtime.set_weights(resnet50=rn, vit=vit, vit_name="vit_base")


def test_every_option_reads_back_its_default_and_round_trips():
    """relax_set_option / relax_get_option over the options table on a fresh handle: the key list of tests/test_options_cpu.py, each key's
    default and one non-default value (no tensor moves)."""
    from relax_vqa_amd.engine import RelaxEngine
    from tests.test_options_cpu import ENV, OPTIONS
    from_env = {key for var, key in ENV.items() if var in os.environ}    # (a poison-mode run of the suite: that key starts as its variable says)
    other = {"given": 5, "floor": 3}
    eng = RelaxEngine(0)
    try:
        for key, (default, rule) in OPTIONS.items():
            initial = eng.get_option(key)
            assert initial == default or key in from_env, key
            kind = rule if isinstance(rule, str) else rule[0]
            if kind == "bool":
                value = 1 - initial
            elif kind == "one_of":
                value = rule[1] if initial == rule[2] else rule[2]
            elif kind == "range":
                value = rule[1] if initial != rule[1] else rule[2]
            else:
                value = other[kind] + (initial == other[kind])
            eng.set_option(key, value)
            assert eng.get_option(key) == value != initial, key
            eng.set_option(key, initial)
            assert eng.get_option(key) == initial, key
        with pytest.raises(RuntimeError, match="relax_set_option: b2b_rows must be 128 or 256"):
            eng.set_option("b2b_rows", 192)
        with pytest.raises(RuntimeError, match="relax_get_option: unknown option 'no_such_option'"):
            eng.get_option("no_such_option")
        assert eng.get_option("profile_events") == 0 and eng.get_option("workspace_mib") == 0    # the two read-only counters, in front of the table
        assert {k: eng.get_option(k) for k in OPTIONS if k not in from_env} == {k: d for k, (d, _) in OPTIONS.items() if k not in from_env}
    finally:
        eng.close()
