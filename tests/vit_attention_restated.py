"""DINO's attention visualisation restated as the parity oracle of csrc/vit_attention_map.hip.

get_last_selfattention (src/extractor/visualise_vit.py:241-250): blocks 0..depth-2 as usual, then the last block's
softmax(q k^T / sqrt(64)) (Block.forward(return_attention=True), :123-127), here at a chosen dtype (fp64 for the accuracy gate).
map_attention_to_original (src/demo_visual.py:12-25) as a literal numpy transcription: a float64 map of zeros, slot values
painted patch by patch, / max * 255, astype(uint8), the colour table looked up (cv2.applyColorMap's role) and addWeighted
computed in float32 and rounded to nearest."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.vit_ref import LN_EPS, preprocess_bgr_u8  # noqa: F401


def _block(sd, t, i, heads, last=False):
    p = f"blocks.{i}."
    B, Nt, dim = t.shape
    hd = dim // heads
    y = F.layer_norm(t, (dim,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], LN_EPS)
    qkv = F.linear(y, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"])
    qkv = qkv.reshape(B, Nt, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    attn = ((q @ k.transpose(-2, -1)) * hd ** -0.5).softmax(dim=-1)
    if last:
        return attn
    y = (attn @ v).transpose(1, 2).reshape(B, Nt, dim)
    t = t + F.linear(y, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
    y = F.layer_norm(t, (dim,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], LN_EPS)
    y = F.gelu(F.linear(y, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"]))
    return t + F.linear(y, sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])


def _prepare(sd, x, patch=16):
    B = x.shape[0]
    t = F.conv2d(x, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=patch)
    t = t.flatten(2).transpose(1, 2)
    return torch.cat((sd["cls_token"].expand(B, -1, -1), t), dim=1) + sd["pos_embed"]


def _depth(sd):
    return 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))


def _cast(np_sd, dtype):
    return {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in np_sd.items()}


@torch.no_grad()
def last_selfattention(np_sd, frags_bgr_u8, heads, dtype=torch.float64):
    """-> [N, heads, 197, 197] at `dtype` (the whole softmax matrix of the last block)."""
    sd = _cast(np_sd, dtype)
    t = _prepare(sd, preprocess_bgr_u8(frags_bgr_u8).to(dtype))
    depth = _depth(sd)
    for i in range(depth - 1):
        t = _block(sd, t, i, heads)
    return _block(sd, t, depth - 1, heads, last=True)


def cls_rows(np_sd, frags_bgr_u8, heads, dtype=torch.float64):
    """-> numpy [N, heads, 197]: the CLS query's row, column 0 included (the engine's [N, heads, 197] output)."""
    return last_selfattention(np_sd, frags_bgr_u8, heads, dtype)[:, :, 0, :].numpy()


@torch.no_grad()
def all_blocks_tokens(np_sd, frags_bgr_u8, heads, dtype=torch.float32):
    """The same block loop run through every block, plus the final norm: [N, 196, dim] patch tokens (oracle.vit_ref's output)."""
    sd = _cast(np_sd, dtype)
    t = _prepare(sd, preprocess_bgr_u8(frags_bgr_u8).to(dtype))
    for i in range(_depth(sd)):
        t = _block(sd, t, i, heads)
    t = F.layer_norm(t, (t.shape[-1],), sd["norm.weight"], sd["norm.bias"], LN_EPS)
    return t[:, 1:]


def add_weighted_f32(a, b):
    """cv2.addWeighted(a, 0.6, b, 0.4, 0) on uint8, in float32: rint(0.6 a + 0.4 b), saturated."""
    r = np.float32(0.6) * a.astype(np.float32) + np.float32(0.4) * b.astype(np.float32)
    return np.clip(np.rint(r), 0, 255).astype(np.uint8)


def map_attention_to_original(original_frame, attention_map, positions, patch_size, lut_bgr):
    """src/demo_visual.py:12-25 with applyColorMap replaced by lut_bgr[level] and the float32 addWeighted above.  positions:
    (y, x) per slot; like the engine (and relax_gather_patches) a slot outside the patch grid paints nothing."""
    H, W = original_frame.shape[:2]
    full_attention = np.zeros_like(original_frame[:, :, 0], dtype=float)
    for (pos, att) in zip(positions, attention_map):
        y, x = int(pos[0]), int(pos[1])
        if not (0 <= y < H // patch_size and 0 <= x < W // patch_size):
            continue
        start_y = y * patch_size
        start_x = x * patch_size
        full_attention[start_y:start_y + patch_size, start_x:start_x + patch_size] = att
    mx = np.max(full_attention)
    if mx > 0:
        full_attention = (full_attention / mx) * 255
        full_attention = full_attention.astype(np.uint8)
    else:                                                   # (undefined in the reference; the engine's documented choice)
        full_attention = np.zeros(full_attention.shape, dtype=np.uint8)
    heatmap = lut_bgr[full_attention]
    return add_weighted_f32(original_frame, heatmap)


def overlay_pixel_loop(frame, values, positions, count, lut_bgr, patch_size=16):
    """The same semantics pixel by pixel (an independent restatement for the CPU test of the numpy one)."""
    H, W = frame.shape[:2]
    ph, pw = H // patch_size, W // patch_size
    owner = {}
    for k in range(min(count, len(values))):
        y, x = int(positions[k][0]), int(positions[k][1])
        if 0 <= y < ph and 0 <= x < pw:
            owner[(y, x)] = float(values[k])
    mx = max(owner.values()) if owner else None
    if len(owner) < ph * pw or H % patch_size or W % patch_size:
        mx = 0.0 if mx is None else max(mx, 0.0)
    out = np.empty_like(frame)
    for yy in range(H):
        for xx in range(W):
            v = owner.get((yy // patch_size, xx // patch_size), 0.0) if yy < ph * patch_size and xx < pw * patch_size else 0.0
            lvl = int(v / mx * 255) if mx > 0 else 0
            for c in range(3):
                out[yy, xx, c] = (6 * int(frame[yy, xx, c]) + 4 * int(lut_bgr[lvl, c]) + 5) // 10
    return out
