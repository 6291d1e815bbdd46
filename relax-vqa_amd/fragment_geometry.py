"""The geometry of the fragment stage, in one place: which (patch_size, target_size, top_n) the HIP kernels are built for
(csrc/fragment.hip: check_geometry states the same rules for the C-ABI).  Pure host code, no GPU, no torch.

  patch_size   8, 16 or 32.  A patch score sums patch_size^2 * 3 bytes; the selection kernel's two 10-bit radix levels hold
               2^20, and 32 * 32 * 3 * 255 = 783360 is the largest maximum that fits, so nothing above 32 can be built on it.
  target_size  a positive multiple of patch_size, at most 448 ((448 / 8)^2 = 3136 slots).
  top_n        0 .. slots, slots = (target_size / patch_size)^2; None = all slots.
"""
from collections import namedtuple

PATCH_SIZES = (8, 16, 32)
MAX_TARGET = 448
BACKBONE_TARGET = 224          # the canvas of the clip paths (the ViT and ResNet-50 take others through their *_canvas methods; VGG-16 takes this one only)

Geometry = namedtuple("Geometry", "patch_size target_size top_n slots tiles_per_row")


def fragment_geometry(patch_size=16, target_size=224, top_n=None):
    """-> Geometry(patch_size, target_size, top_n, slots, tiles_per_row); ValueError naming the offending value otherwise."""
    for name, v in (("patch_size", patch_size), ("target_size", target_size)) + ((("top_n", top_n),) if top_n is not None else ()):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"fragment geometry: {name}={v!r} is not an integer")
    patch_size, target_size = int(patch_size), int(target_size)
    if patch_size > 32:
        raise ValueError(f"fragment geometry: patch_size={patch_size}: scores of patch_size^2 * 3 bytes do not fit the selection's "
                         f"20-bit radix above 32 (built: {PATCH_SIZES})")
    if patch_size not in PATCH_SIZES:
        raise ValueError(f"fragment geometry: patch_size={patch_size} is not built (one of {PATCH_SIZES})")
    if target_size <= 0 or target_size % patch_size or target_size > MAX_TARGET:
        raise ValueError(f"fragment geometry: target_size={target_size} must be a positive multiple of patch_size={patch_size}, "
                         f"at most {MAX_TARGET}")
    per_row = target_size // patch_size
    slots = per_row * per_row
    top_n = slots if top_n is None else int(top_n)
    if not 0 <= top_n <= slots:
        raise ValueError(f"fragment geometry: top_n={top_n} must be in [0, {slots}] at patch_size={patch_size}, target_size={target_size}")
    return Geometry(patch_size, target_size, top_n, slots, per_row)


def backbone_geometry(patch_size=16, top_n=None, target_size=None):
    """The geometry of a clip path that feeds the backbones (extract_clip, clip_vectors, full_clip_vector(s)): the canvas is 224 x 224, the
    one all three backbones take and the one the reference's feature files are cut at, so passing target_size at all is refused.  Other
    canvases have methods of their own: RelaxEngine.fragment_vit_vectors, fragment_resnet_vectors and fragment_canvas_vectors take
    target_size (the ViT any multiple of the patch size, ResNet-50 multiples of 32: resnet50_canvas_geometry)."""
    if target_size is not None:
        raise ValueError(f"target_size={target_size}: the clip paths cut {BACKBONE_TARGET} x {BACKBONE_TARGET} canvases, the only input the "
                         "backbones take; resizing another canvas before them is out of scope (fragment_pairs takes target_size)")
    return fragment_geometry(patch_size, BACKBONE_TARGET, top_n)


def overlay_slot_rule(fragment_patch, vit_patch):
    """How a slot of a fragment cut at fragment_patch gets its value from a ViT of patch size vit_patch: -> tokens per slot side
    (1 = one token per slot).  The rule: where a ViT with the fragment's patch size exists (8, 16), that model must be the one
    loaded - one source patch per token, painted one to one; a slot of four tokens of a finer model is refused, the matching
    fragment is one argument away.  A 32 x 32 fragment has no such model: its slot takes the mean of the head-mean attention of
    the (32 / vit_patch)^2 tokens it covers - the reshape-and-mean of the reference's get_activation_png (src/demo_visual.py:41-60)."""
    if fragment_patch == vit_patch:
        return 1
    if fragment_patch == 32 and vit_patch in (8, 16):
        return 32 // vit_patch
    raise ValueError(f"the overlay paints one slot of the fragment per ViT token: the fragment's patch size is {fragment_patch}, the loaded "
                     f"model has patch size {vit_patch}; cut the fragment with patch_size={vit_patch} (or 32, a slot then takes the mean "
                     f"of its tokens), or load a patch-{fragment_patch} model")
