"""Counterpart of the reference driver src/main_fragment_pool.py (fragments + `pool` features of one backbone, the
driver that produces the ViT half of the fragment features): same names, argument order and return arity, on the HIP
engine.  It differs from main_fragment_layerstack only in get_deep_feature's layer names ('pool' | 'last_layer',
reference :83-111) and the two-argument process_video_feature (:114-143).  fragment_pair's opt-in `write_png` keyword
(default off) writes the pair's PNG files, as in main_fragment_layerstack.  The fragment functions take the reference's patch_size /
target_size / top_n arguments at every supported geometry (fragment_geometry.py), as they do there."""
from .main_fragment_layerstack import (concatenate_features, extract_important_patches, flow_to_rgb,  # noqa: F401
                                       fragment_pair, get_original_frame_patches, get_patch_diff, merge_fragments,
                                       process_patches)
from .main_residual_fragment import get_deep_feature, process_video_feature  # noqa: F401
