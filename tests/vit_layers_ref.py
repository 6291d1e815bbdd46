"""CPU restatement of the reference ViT's get_intermediate_layers (helper of tests/test_vit_layers_cpu.py and tests/test_gpu_vit_layers.py).

src/extractor/visualise_vit_layer.py:252-260: prepare_tokens, then the blocks, and after each block i with depth - i <= n the final norm
of the stream as it stands.  The block loop is tests/vit_canvas_ref.forward_canvas' (itself pinned to the reference's class), with the
norm applied at the tapped blocks; tests/golden/vit_layers.npz pins this file against the reference's own method
(tools/make_vit_layers_golden.py).  `dtype`: the arithmetic of the whole forward (torch.float64 for the distance-from-fp64 gates)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import vit_ref
from tests import vit_canvas_ref


@torch.no_grad()
def intermediate_layers(sd, x, heads, patch, n=1, dtype=torch.float32):
    """x [B,3,Hc,Wc] -> list of min(n, depth) tensors [B,ntok,dim] in block order (n > depth returns every block, as the reference's
    `len(self.blocks) - i <= n` does)"""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    x = x.to(dtype)
    B = x.shape[0]
    t = F.conv2d(x, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=patch)
    gh, gw = t.shape[-2:]
    t = t.flatten(2).transpose(1, 2)
    t = torch.cat((sd["cls_token"].expand(B, -1, -1), t), dim=1) + vit_canvas_ref.interpolate_pos(sd["pos_embed"], gh, gw, dtype)
    dim = t.shape[-1]
    hd = dim // heads
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    output = []
    for i in range(depth):
        p = f"blocks.{i}."
        y = F.layer_norm(t, (dim,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], vit_ref.LN_EPS)
        qkv = F.linear(y, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"])
        qkv = qkv.reshape(B, -1, 3, heads, hd).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        attn = ((q @ k.transpose(-2, -1)) * hd ** -0.5).softmax(dim=-1)
        y = (attn @ v).transpose(1, 2).reshape(B, -1, dim)
        t = t + F.linear(y, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
        y = F.layer_norm(t, (dim,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], vit_ref.LN_EPS)
        y = F.gelu(F.linear(y, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"]))
        t = t + F.linear(y, sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
        if depth - i <= n:
            output.append(F.layer_norm(t, (dim,), sd["norm.weight"], sd["norm.bias"], vit_ref.LN_EPS))
    return output


def pooled(tap):
    """one tap [B,ntok,dim] (tensor or numpy) -> [B,3*dim] in the tap's precision: mean | max | population std over the patch tokens tap[:, 1:]"""
    t = tap.numpy() if isinstance(tap, torch.Tensor) else np.asarray(tap)
    t = t[:, 1:]
    return np.concatenate([t.mean(axis=1), t.max(axis=1), t.std(axis=1)], axis=1)
