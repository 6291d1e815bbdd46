"""Counterpart of src/extractor/visualise_vgg.py (reference): layer-stack activations of VGG-16.

Reference: process_video_frame(video_name, image_path, all_layers, qp) runs one full forward per selector through a forward
hook on vgg16.features[i] (:22-58, :60-105).  Here ONE forward on the GPU yields all 13 taps.  torchvision's ReLU(inplace=True)
behind every convolution rectifies the hooked tensor before the reference copies it, so the taps are post-ReLU."""
import os

import numpy as np
import torch

from .. import runtime
from .visualise_resnet import LayerStackActivations, _frame_number

# the reference's selectors (src/main_fragment_layerstack.py:103): the indices of the 13 convolutions in vgg16.features
ALL_LAYERS = [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]
LAYER_INDEX = {idx: i for i, idx in enumerate(ALL_LAYERS)}


def process_fragment_array(frag_bgr_u8, all_layers=ALL_LAYERS):
    """Array form: uint8 [224,224,3] BGR -> dict features-index -> [C,H,W], with `.pooled` = the fp32 [4224] spatial means
    (when all 13 taps are asked for, in the reference's order)."""
    eng = runtime.ensure_vgg16()
    idx = []
    for name in all_layers:
        if name not in LAYER_INDEX:
            raise ValueError(f"unknown VGG-16 layer selector {name!r} (the convolutions are features[{ALL_LAYERS}])")
        idx.append(LAYER_INDEX[name])
    ls, _, taps = eng.vgg16_features(torch.from_numpy(np.ascontiguousarray(frag_bgr_u8)), layer_stack=True, pool=False, taps=idx)
    out = LayerStackActivations()
    for name, i in zip(all_layers, idx):
        out[name] = taps[i][0].cpu().numpy()
    if list(all_layers) == ALL_LAYERS:
        out.pooled = ls[0].cpu().numpy()
    return out


def process_video_frame(video_name, image_path, all_layers, qp):
    filename = os.path.basename(image_path)
    frame_number = _frame_number(filename)
    img = runtime.to_model_input(runtime.read_image_bgr(image_path), "vgg16")
    activations = process_fragment_array(img, all_layers)
    combined = "vgg16_feature_map_original" if qp == "original_ugc" else f"vgg16_feature_map_qp_{qp}"
    return activations, f"../features/vgg16/{video_name}/frame_{frame_number}_{combined}.npy"
