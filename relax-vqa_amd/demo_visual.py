"""Counterpart of src/demo_visual.py (reference): where the ViT looked, painted onto the source frame.

get_activation_png (:41-60) averages the last block's CLS attention over heads and over each 16 x 16 block (one value per
fragment slot); map_attention_to_original (:12-25) writes each slot's value back onto the frame patch it was cut from,
normalises by the maximum, colours it with a jet table and blends it 0.6 / 0.4 with the frame (csrc/vit_attention_map.hip).
Nothing here plots or writes files: the functions return arrays.  RelaxEngine.attention_overlays does the whole __main__
(:86-128) for a clip on the GPU."""
import numpy as np
import torch

from . import runtime
from .fragment_geometry import fragment_geometry
from .extractor import visualise_vit


def map_attention_to_original(original_frame, attention_map, positions, patch_size, lut=None):
    """original_frame uint8 [H,W,3] BGR; attention_map: one value per slot (patch_means.flatten()); positions: (y, x) patch
    coordinates per slot, in units of patch_size (8, 16 or 32) pixels ((-1, -1) or out-of-range slots paint nothing) -> uint8
    [H,W,3].  lut: see colormap.py.  The slots of a 224 x 224 canvas are taken ((224 / patch_size)^2: 784 / 196 / 49); a longer list
    is cut there, as it was at 196.  With a ViT loaded, patch_size has to go with it (RelaxEngine.attention_overlay)."""
    geo = fragment_geometry(patch_size, 224)
    eng = runtime.get_engine()
    values = np.asarray(attention_map, dtype=np.float32).reshape(-1)
    pos = np.asarray(positions, dtype=np.int64).reshape(-1, 2)
    slots = geo.slots
    count = min(len(values), len(pos), slots)          # zip(positions, attention_map) stops at the shorter one
    pos_full = np.full((1, slots, 2), -1, dtype=np.int32)
    val_full = np.zeros((1, slots), dtype=np.float32)
    pos_full[0, :count] = np.clip(pos[:count], -1, np.iinfo(np.int32).max)
    val_full[0, :count] = values[:count]
    frame = torch.from_numpy(np.ascontiguousarray(original_frame)[None])
    out = eng.attention_overlay(frame, torch.from_numpy(pos_full), torch.tensor([count], dtype=torch.int32),
                                torch.from_numpy(val_full), lut=lut, patch_size=geo.patch_size)
    return out[0].cpu().numpy()


def get_activation_png(attention, residual_name, patch_size=16, img_dim=224):
    """attention fp32 [heads, 224, 224] (visualise_vit.visualize_attention) -> patch_means [14, 14]: the head mean, then the
    mean of each 16 x 16 block.  The reference's plot is not drawn."""
    patch_per_dim = img_dim // patch_size
    head_mean = np.mean(attention, axis=0).reshape((patch_per_dim, patch_size, patch_per_dim, patch_size))
    return head_mean.mean(axis=(1, 3)).reshape((patch_per_dim, patch_per_dim))


def process_frame_with_attention(imp_path_or_array, positions, residual_name, original_frame, name_model="vit_base"):
    """The fragment (a PNG path or a uint8 BGR array; not 224 x 224: LANCZOS to 224) through the ViT, its head-mean patch
    attention mapped onto original_frame at `positions` -> uint8 [H,W,3] (the reference shows it with plt.show() instead and
    reads original_frame from a module global)."""
    img = imp_path_or_array
    if not isinstance(img, np.ndarray):
        img = runtime.read_image_bgr(img)
    img = runtime.to_model_input(img, "vit")
    model = visualise_vit.VitGenerator(name_model, 16, None, evaluate=True, random=False)
    attentions = visualise_vit.visualize_attention(model, img, 16, None)
    patch_means = get_activation_png(attentions, residual_name)
    return map_attention_to_original(original_frame, patch_means.flatten(), positions, 16)
