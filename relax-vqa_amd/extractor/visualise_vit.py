"""Counterpart of src/extractor/visualise_vit.py (reference): DINO ViT last-block attention maps.

Reference: get_last_selfattention runs blocks 0..10 and returns block 11's softmax(q k^T / 8) (:241-250, :123-127);
visualize_attention keeps the CLS query's row against the 196 patches for every head and nearest-upsamples it to
[heads, H, W] at the (cropped) size of its input (:353-369); process_video_frame resizes to 224 x 224 first and returns it as a per-head dict (:414-431, :457-500).  The reference rebuilds
the model for every image and runs a full forward; here the weights live in the engine and the forward stops after block 11's
qkv GEMM (RelaxEngine.vit_attention)."""
import os

import numpy as np
import torch

from .. import runtime
from .visualise_resnet import _frame_number
from .visualise_vit_layer import VitGenerator  # noqa: F401  (the same generator handle as the token extractor)


def _attention(model, frag_bgr_u8):
    eng = runtime.ensure_vit(model.name_model, model.patch_size)
    frags = torch.from_numpy(np.ascontiguousarray(frag_bgr_u8)) if isinstance(frag_bgr_u8, np.ndarray) else frag_bgr_u8
    return eng.vit_attention(frags)


def visualize_attention(model, img, patch_size, device):
    """img: uint8 [H,W,3] BGR of any size at least one patch (a fragment; a frame, as it is or through runtime.to_model_input(.., "vit")).
    As the reference (:355-357) the image is cropped to multiples of the patch size, img[:H - H % p, :W - W % p], and runs at that size
    (the position table resampled onto its grid) -> fp32 numpy [heads, gh*p, gw*p]: attn[0, :, 0, 1:] as [heads, gh, gw] ([heads, 14, 14]
    at 224 x 224 and patch 16), each value repeated over its patch (mode="nearest")."""
    if patch_size != model.patch_size:
        raise ValueError(f"visualize_attention: patch_size {patch_size}, the model was built with {model.patch_size}")
    if not torch.is_tensor(img):
        img = np.asarray(img)
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"visualize_attention: img must be [H,W,3], got {tuple(img.shape)}")
    gh, gw = img.shape[0] // patch_size, img.shape[1] // patch_size
    img = img[:gh * patch_size, :gw * patch_size]
    att = _attention(model, img).cpu().numpy()[0]                    # [heads, npatch]
    nh = att.shape[0]
    att = att.reshape(nh, gh, gw)
    return np.repeat(np.repeat(att, patch_size, axis=1), patch_size, axis=2)


def get_activation_npy(npy_path, video_name, frame_number, qp, fig_name, combined_name, attention):
    """-> (dict head index -> [224, 224], the reference's .npy path string); nothing is written (as in the reference, :414-431)."""
    activations_dict = {i: attention[i] for i in range(attention.shape[0])}
    frame_activation_npy_path = f'../features/vit/{video_name}/frame_activation_{frame_number}_{combined_name}.npy'
    return activations_dict, frame_activation_npy_path


def process_video_frame(image_path, video_name, qp, model, patch_size, device):
    """image_path: a PNG path (its name gives the frame number, as in the reference) or a uint8 [H,W,3] BGR array (frame number 0).
    An image that is not 224 x 224 goes through the reference's LANCZOS resize (:466-469) on the GPU.
    -> (dict head -> fp32 [224, 224], the reference's .npy path string)."""
    if isinstance(image_path, np.ndarray):
        img, frame_number = image_path, 0
    else:
        frame_number = _frame_number(os.path.basename(image_path))
        img = runtime.read_image_bgr(image_path)
    img = runtime.to_model_input(img, "vit")
    attention = visualize_attention(model, img, patch_size, device)
    combined_name = "vit_feature_map_original" if qp == "original" else f"vit_feature_map_qp_{qp}"
    return get_activation_npy(None, video_name, frame_number, qp, combined_name, combined_name, attention)
