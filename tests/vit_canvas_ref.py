"""CPU fp32 restatement of the reference ViT on any canvas (helper of tests/test_vit_canvas_cpu.py and tests/test_gpu_vit_canvas.py).

prepare_tokens with interpolate_pos_encoding as src/extractor/visualise_vit_layer.py:197-232 has it - the position table resampled by
F.interpolate(scale_factor=((gh + 0.1) / side, (gw + 0.1) / side), mode='bicubic'), the table itself when the grid is the table's
(:200-201) -, then the block arithmetic of oracle.vit_ref.forward_tokens, line for line.  tests/golden/vit_canvas.npz pins it against the
reference's own class (tools/make_vit_canvas_golden.py)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import vit_ref


def preprocess_bgr_u8(img_bgr_u8):
    """uint8 [N,Hc,Wc,3] BGR -> fp32 [N,3,Hc,Wc] RGB in [0,1] (oracle.vit_ref.preprocess_bgr_u8 without its 224)"""
    x = torch.as_tensor(np.ascontiguousarray(np.asarray(img_bgr_u8)[..., ::-1]))
    return x.permute(0, 3, 1, 2).to(torch.float32).div(255)


def interpolate_pos(pos_embed, gh, gw, dtype=torch.float32):
    """pos_embed [1, 1 + side^2, dim] -> [1, 1 + gh*gw, dim]: the reference's interpolate_pos_encoding for a gh x gw patch grid"""
    pos_embed = pos_embed.to(dtype)
    n = pos_embed.shape[1] - 1
    side = int(math.sqrt(n))
    if gh * gw == n and gh == gw:
        return pos_embed
    dim = pos_embed.shape[-1]
    table = pos_embed[:, 1:].reshape(1, side, side, dim).permute(0, 3, 1, 2)
    table = F.interpolate(table, scale_factor=((gh + 0.1) / side, (gw + 0.1) / side), mode="bicubic")
    assert tuple(table.shape[-2:]) == (gh, gw), (table.shape, gh, gw)
    return torch.cat((pos_embed[:, :1], table.permute(0, 2, 3, 1).reshape(1, -1, dim)), dim=1)


@torch.no_grad()
def forward_canvas(sd, x, heads, patch):
    """x fp32 [B,3,Hc,Wc] -> (cls [B,dim], tokens [B,npatch,dim], the last block's attention [B,heads,ntok,ntok])"""
    B = x.shape[0]
    t = F.conv2d(x, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=patch)
    gh, gw = t.shape[-2:]
    t = t.flatten(2).transpose(1, 2)
    t = torch.cat((sd["cls_token"].expand(B, -1, -1), t), dim=1) + interpolate_pos(sd["pos_embed"], gh, gw)
    dim = t.shape[-1]
    hd = dim // heads
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    last = None
    for i in range(depth):
        p = f"blocks.{i}."
        y = F.layer_norm(t, (dim,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], vit_ref.LN_EPS)
        qkv = F.linear(y, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"])
        qkv = qkv.reshape(B, -1, 3, heads, hd).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        attn = ((q @ k.transpose(-2, -1)) * hd ** -0.5).softmax(dim=-1)
        last = attn
        y = (attn @ v).transpose(1, 2).reshape(B, -1, dim)
        t = t + F.linear(y, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
        y = F.layer_norm(t, (dim,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], vit_ref.LN_EPS)
        y = F.gelu(F.linear(y, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"]))
        t = t + F.linear(y, sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
    t = F.layer_norm(t, (dim,), sd["norm.weight"], sd["norm.bias"], vit_ref.LN_EPS)
    return t[:, 0], t[:, 1:], last


def pooled(tokens):
    """tokens [B,npatch,dim] (numpy) -> [B,3*dim]: mean | max | population std over the patch tokens (src/main_fragment_pool.py:124-133)"""
    return np.concatenate([tokens.mean(axis=1), tokens.max(axis=1), tokens.std(axis=1)], axis=1).astype(np.float32)


# ---- tests/golden/vit_canvas.npz (tools/make_vit_canvas_golden.py) ---------------------------------------------------------------------
def golden_input(shape, seed):
    return np.random.default_rng(int(seed)).integers(0, 256, tuple(int(v) for v in shape), dtype=np.uint8)


def golden_state_dict(z, patch):
    """the fp32 torch state dict of one patch size from the loaded fixture: the shared keys w.<key> and that patch size's w<patch>.<key>"""
    sd = {k[2:]: z[k] for k in z.files if k.startswith("w.")}
    sd.update({k[len(f"w{patch}."):]: z[k] for k in z.files if k.startswith(f"w{patch}.")})
    return {k: torch.from_numpy(np.asarray(v).astype(np.float32)) for k, v in sd.items()}
