"""Counterpart of src/extractor/visualise_vit_layer.py (reference): DINO ViT patch tokens.

Reference: VitGenerator(name_model, patch_size, device, evaluate=True, random=False, verbose=False) builds the model
and loads hub weights (:263-329); process_video_frame(image_path, video_name, qp, model, patch_size, device) returns
the final-norm patch tokens [196, dim] (:447-500; [784, dim] at patch size 8).  The reference rebuilds the generator for every frame
(src/main_fragment_layerstack.py:118); here the weights live in the engine and the generator is a light handle."""
import os

import numpy as np
import torch

from .. import runtime, synth
from .visualise_resnet import _frame_number


class VitGenerator(object):
    def __init__(self, name_model, patch_size, device=None, evaluate=True, random=False, verbose=False):
        if name_model not in ("vit_tiny", "vit_small", "vit_base"):
            raise ValueError(f"No model found with {name_model}")   # the reference raises a bare string here (:291)
        if patch_size not in (8, 16):
            raise ValueError(f"patch_size {patch_size}: DINO checkpoints exist for 8 and 16 (:309-320)")
        self.name_model = name_model
        self.patch_size = patch_size
        self.device = device
        self.evaluate = evaluate
        self.verbose = verbose
        if random:
            runtime.set_weights(vit=synth.vit_state_dict(name_model, patch=patch_size), vit_name=name_model, vit_patch=patch_size)
        else:
            runtime.ensure_vit(name_model, patch_size)   # ValueError naming both sizes if the configured weights have the other one

    def tokens(self, frag_bgr_u8):
        eng = runtime.ensure_vit(self.name_model, self.patch_size)
        t, _ = eng.vit_features(torch.from_numpy(np.ascontiguousarray(frag_bgr_u8)), tokens=True, pooled=False)
        return t

    def __call__(self, frag_bgr_u8):
        """frag_bgr_u8 uint8 [N,Hc,Wc,3] (any canvas: VisionTransformer.forward interpolates the position table, :197-232) -> (None, tokens
        [N,(Hc//p)*(Wc//p),dim]: [N,196,dim] at 224 x 224, [N,784,dim] at patch size 8); the cls token is not part of the hot path."""
        return None, self.tokens(frag_bgr_u8)


    def get_intermediate_layers(self, x, n=1):
        """VisionTransformer.get_intermediate_layers (:252-260): x uint8 [N,Hc,Wc,3] BGR -> list of n tensors [N,ntok,dim], the final norm of
        the output of each of the last n blocks (row 0 the CLS token), in block order; one forward."""
        eng = runtime.ensure_vit(self.name_model, self.patch_size)
        t = eng.vit_intermediate_layers(torch.from_numpy(np.ascontiguousarray(x)), n=n, tokens=True, cls=False, pooled=False)["tokens"]
        return list(t.unbind(0))

    def cls_token(self, x):
        """forward's first output (:234-239, x[:, 0] after the final norm): x uint8 [N,Hc,Wc,3] BGR -> [N,dim]"""
        eng = runtime.ensure_vit(self.name_model, self.patch_size)
        return eng.vit_intermediate_layers(torch.from_numpy(np.ascontiguousarray(x)), n=1, tokens=False, cls=True, pooled=False)["cls"][0]


def process_fragment_array(frag_bgr_u8, model):
    """frag_bgr_u8 uint8 [Hc,Wc,3] or [1,Hc,Wc,3], any canvas -> fp32 numpy [(Hc//p)*(Wc//p), dim]"""
    return model.tokens(frag_bgr_u8)[0].cpu().numpy()


def process_video_frame(image_path, video_name, qp, model, patch_size, device):
    filename = os.path.basename(image_path)
    frame_number = _frame_number(filename)
    img = runtime.to_model_input(runtime.read_image_bgr(image_path), "vit")
    feats = process_fragment_array(img, model)
    combined = "vit_feature_map_original" if qp == "original" else f"vit_feature_map_qp_{qp}"
    return feats, f"../features/vit/{video_name}/frame_attention_{frame_number}_{combined}.npy"
