"""The reference drivers' per-pair PNG files, written from the device (src/main_fragment_layerstack.py:310,325,
src/main_residual.py:230,241, src/main_residual_fragment.py:213, src/demo_test.py:120,135 - cv2.imwrite).  The images are the
engine's own arrays (residual_resize, fragment_pairs, optical_flow, fragment_image, merge_fragments, attention_overlays); all
images of a clip go through a few encode calls (one per image size), never one launch per file."""
import os

NAMES = ("residual", "residual_imp", "ori_frag", "residual_of", "residual_of_imp", "residual_merged_frag")


def example_set_arrays(engine, frames, flow=True, overlays=None, flow_params=None):
    """frames uint8 [T,2,H,W,3] -> {suffix: uint8 [T,h,w,3] device tensor} of the files write_example_set writes.
    flow_params: a dict of RelaxEngine.optical_flow's keywords (None = the reference's literals)."""
    frames = engine._dev_u8(frames)
    fr = engine.fragment_pairs(frames)
    out = {"residual": engine.residual_resize(frames, bilinear=False, lanczos=False, want_residual=True)[2],
           "residual_imp": fr["diff_frag"], "ori_frag": fr["ori_frag"]}
    flow_images = None
    if flow:
        flow_images = engine.clip_flow_images(frames, flow_params)
        fl = engine.fragment_image(flow_images)
        out["residual_of"] = flow_images
        out["residual_of_imp"] = fl["frag"]
        out["residual_merged_frag"] = engine.merge_fragments(fr["diff_frag"], fl["frag"])
    if overlays is not None:
        if overlays not in engine.OVERLAY_FRAGMENTS:
            raise ValueError(f"overlays must be one of {engine.OVERLAY_FRAGMENTS}, got {overlays!r}")
        out[f"{overlays}_overlay"] = engine.attention_overlays(frames, overlays, flow_images=flow_images, flow_params=flow_params)["overlay"]
    return out


def write_example_set(engine, frames, directory, video_name, flow=True, overlays=None, numbers=None):
    """Writes, for every pair t of the clip frames [T,2,H,W,3], the reference's files `{video_name}_{n}_{suffix}.png` with the
    suffixes NAMES (the three flow kinds only with flow=True) and, when `overlays` names one of
    RelaxEngine.OVERLAY_FRAGMENTS, `{video_name}_{n}_{overlays}_overlay.png`.  n: numbers[t], the sampled frame's number as
    sampling.frame_pair_paths reads it back (default t + 1).  -> {suffix: [path per pair]}; the arrays are
    example_set_arrays'."""
    arrays = example_set_arrays(engine, frames, flow=flow, overlays=overlays)
    T = frames.shape[0]
    numbers = list(range(1, T + 1)) if numbers is None else list(numbers)
    if len(numbers) != T:
        raise ValueError(f"{len(numbers)} numbers for {T} pairs")
    os.makedirs(directory, exist_ok=True)
    paths = {s: [os.path.join(directory, f"{video_name}_{n}_{s}.png") for n in numbers] for s in arrays}
    by_size = {}
    for s, a in arrays.items():
        by_size.setdefault(tuple(a.shape[1:]), []).append(s)
    for suffixes in by_size.values():            # one encode call per image size: the full-size kinds, the 224 x 224 kinds
        images = [arrays[s][t] for s in suffixes for t in range(T)]
        engine.write_png([paths[s][t] for s in suffixes for t in range(T)], images)
    return paths


def write_for_driver(engine, frames, write_png, flow=True):
    """The drivers' opt-in `write_png` keyword: None (nothing is written) or (directory, video_name[, numbers]) -> the files of
    write_example_set for the driver's pairs."""
    if write_png is None:
        return None
    directory, video_name = write_png[0], write_png[1]
    numbers = write_png[2] if len(write_png) > 2 else None
    return write_example_set(engine, frames, directory, video_name, flow=flow, numbers=numbers)
