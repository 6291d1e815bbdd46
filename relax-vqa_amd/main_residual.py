"""Counterpart of the reference driver src/main_residual.py (the fragment-free residual ablation: the WHOLE residual image of
a frame pair - not its top-196 fragment - is resized to 224x224 and pooled): same function names, argument order and return
arity as that file, running on the HIP engine.

  get_deep_feature(network_name, video_name, image_path, qp, layer_name)      (reference :83-115)
  process_video_feature(video_feature, network_name)                          (reference :118-156) -> 2051 / 4099 / 3*dim
  flow_to_rgb(flow)                                                           (reference :158-171)
  process_pair(img_original, img_next, network_name, residual_name, layer_name='pool')
      one iteration of the loop at :221-252 on arrays: the reference writes the residual to `_residual.png` /
      `_residual_of.png` and hands the path to get_deep_feature; here the frame difference is taken inside the resize
      (`relax_resize_residual`: the pair is read once) and the flow image goes through `relax_resize_frames`.

Activations returned by get_deep_feature / process_pair carry the vector the GPU pooled as `.pooled`; process_video_feature
uses it.  Plain arrays (activations recorded earlier, e.g. the per-frame .npy files) are reduced with the numpy calls of the
reference."""
import numpy as np
import torch

from . import runtime
from .extractor import visualise_resnet_layer, visualise_vgg_layer
from .main_fragment_layerstack import flow_to_rgb  # noqa: F401  (same behaviour in every driver)

RESIDUAL_NAMES = ("frame_diff", "optical_flow")
LAYER_NAMES = ("pool", "last_layer")
NETWORK_NAMES = ("resnet50", "vgg16", "vit")


class TokenActivation(np.ndarray):
    """ndarray [196,dim] like the reference returns for the ViT, plus `.pooled`: the fp32 [3*dim] token mean | max | std."""
    pooled = None


def _check_names(network_name, layer_name):
    if network_name not in NETWORK_NAMES:
        raise NotImplementedError(f"network {network_name!r} is out of scope")
    if network_name != "vit" and layer_name not in LAYER_NAMES:
        raise ValueError(f"unknown layer_name {layer_name!r}")      # the reference hits an unbound local here


def _activation(network_name, image, layer_name):
    """image uint8 [224,224,3] -> the activation the reference's extractor returns for it."""
    if network_name == "resnet50":
        return visualise_resnet_layer.process_fragment_array(image, "resnet50.avgpool" if layer_name == "pool" else "resnet50.layer4[2]")
    if network_name == "vgg16":
        return visualise_vgg_layer.process_fragment_array(image, "fc2" if layer_name == "pool" else 28)
    tokens, pooled = runtime.ensure_vit("vit_base").vit_features(torch.from_numpy(np.ascontiguousarray(image)), tokens=True, pooled=True)
    out = tokens[0].cpu().numpy().view(TokenActivation)
    out.pooled = pooled[0].cpu().numpy()
    return out


def get_deep_feature(network_name, video_name, image_path, qp, layer_name):
    """-> (png_path, npy_path, frame_npy) (reference :83-115); image_path: an image file or a uint8 [H,W,3] BGR image (the
    residual image).  A whole image is resized the way the extractors do it, PIL-exact on the GPU."""
    _check_names(network_name, layer_name)
    png_path = f"../visualisation/{network_name}/{video_name}/"
    npy_path = f"../features/{network_name}/{video_name}/"
    image = runtime.read_image_bgr(image_path) if isinstance(image_path, str) else image_path
    return png_path, npy_path, _activation(network_name, runtime.to_model_input(image, network_name), layer_name)


# Opt-in, default off: (directory, video_name, [n]) makes process_pair also write the pair's files as the reference's cv2.imwrite
# calls leave them (:230, :241; visualisation.write_example_set, encoded on the GPU).  A module flag, not a keyword: process_pair
# keeps the reference's parameter list.  Its return value does not change.
WRITE_PNG = None


def process_pair(img_original, img_next, network_name, residual_name, layer_name="pool"):
    """One (frame, next frame) pair -> residual_npy, the activation the loop body at reference :221-252 appends."""
    if residual_name not in RESIDUAL_NAMES:
        raise ValueError(f"residual_name must be one of {RESIDUAL_NAMES}, got {residual_name!r}")
    _check_names(network_name, layer_name)
    eng = runtime.get_engine()
    frames = torch.from_numpy(np.stack([np.ascontiguousarray(img_original), np.ascontiguousarray(img_next)])[None])
    vit = network_name == "vit"
    if WRITE_PNG is not None:
        from . import visualisation
        visualisation.write_for_driver(eng, frames, WRITE_PNG)
    if residual_name == "frame_diff":
        bil, lan, _ = eng.residual_resize(frames, bilinear=not vit, lanczos=vit)
    else:
        bil, lan = eng.resize_frames(eng.optical_flow(frames)[1], bilinear=not vit, lanczos=vit)
    return _activation(network_name, (lan if vit else bil)[0].cpu().numpy(), layer_name)


def token_stats(frame):
    """[tokens, dim] -> [3*dim] mean | max | population std over the tokens (reference :128-136)."""
    return np.hstack([np.mean(frame, axis=0), np.max(frame, axis=0), np.std(frame, axis=0)])


def squeezed(frame):
    """The 'pool' activation as a vector; 'last_layer' maps ([2048,7,7]) go through axis-0 statistics in the reference and
    give a ragged stack that nothing downstream reads: not reproduced."""
    frame = np.squeeze(np.asarray(frame))
    if frame.ndim != 1:
        raise NotImplementedError("process_video_feature pools 'pool' activations; 'last_layer' is a visualisation tap")
    return frame


def process_video_feature(video_feature, network_name):
    """list of per-frame activations -> [T, 3*dim] (vit), [T, 2051] (resnet50 pool) or [T, 4099] (vgg16 fc2) (reference :118-156)."""
    rows = []
    for frame in video_feature:
        pooled = getattr(frame, "pooled", None)
        if network_name == "vit":
            rows.append(pooled if pooled is not None else token_stats(frame))
        else:
            frame = squeezed(frame)
            rows.append(pooled if pooled is not None else
                        np.hstack([frame, np.mean(frame, axis=0), np.max(frame, axis=0), np.std(frame, axis=0)]))
    return np.array(rows)
