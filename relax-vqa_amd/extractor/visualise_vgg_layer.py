"""Counterpart of src/extractor/visualise_vgg_layer.py (reference): one hooked VGG-16 layer, used with 'fc2' for the 'pool'
features (src/main_fragment_layerstack.py:106-108).  Selectors: 'fc1' (classifier[0]), 'fc2' (classifier[3]) or the index of a
convolution in vgg16.features (:51-60).  Every activation is post-ReLU (torchvision's in-place ReLU follows each hooked module)."""
import os

import numpy as np
import torch

from .. import runtime
from .visualise_resnet import _frame_number
from .visualise_vgg import LAYER_INDEX


class PoolActivation(np.ndarray):
    """ndarray [4096] like the reference returns for 'fc2', plus `.pooled`: the fp32 [4099] vector (fc2 + mean/max/std)."""
    pooled = None


def process_fragment_array(frag_bgr_u8, layer_name="fc2"):
    eng = runtime.ensure_vgg16()
    x = torch.from_numpy(np.ascontiguousarray(frag_bgr_u8))
    if layer_name == "fc2":
        _, pool = eng.vgg16_features(x, layer_stack=False, pool=True)
        p = pool[0].cpu().numpy()
        out = p[:4096].copy().view(PoolActivation)
        out.pooled = p
        return out
    if layer_name == "fc1":
        _, _, taps = eng.vgg16_features(x, layer_stack=False, pool=False, taps=[13])
        return taps[13][0].cpu().numpy()
    if isinstance(layer_name, (int, np.integer)) and int(layer_name) in LAYER_INDEX:
        i = LAYER_INDEX[int(layer_name)]
        _, _, taps = eng.vgg16_features(x, layer_stack=False, pool=False, taps=[i])
        return taps[i][0].cpu().numpy()
    raise ValueError(f"unknown VGG-16 layer selector {layer_name!r}")


def process_video_frame(video_name, image_path, layer_name, qp):
    filename = os.path.basename(image_path)
    frame_number = _frame_number(filename)
    img = runtime.to_model_input(runtime.read_image_bgr(image_path), "vgg16")
    arr = process_fragment_array(img, layer_name)
    combined = "vgg16_feature_map_original" if qp == "original_ugc" else f"vgg16_feature_map_qp_{qp}"
    return arr, f"../features/vgg16/{video_name}/frame_{frame_number}_{combined}.npy"
