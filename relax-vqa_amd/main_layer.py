"""Counterpart of the reference driver src/main_layer.py (whole-frame *pool* features: every sampled frame is resized to
224x224 and the ResNet-50 avgpool vector, the VGG-16 fc2 vector or the ViT token statistics are kept), running on the HIP
engine.

  get_deep_feature(network_name, video_name, image_path, qp, layer_name)      five arguments (reference :81-113)
  process_video_feature(video_feature, network_name)                          two arguments (reference :116-148)

Unlike src/main_residual.py this driver keeps the squeezed activation alone for the CNNs - [T, 2048] / [T, 4096], no
mean / max / std columns (:135-137); the ViT rows are [T, 3*dim] as everywhere."""
import numpy as np

from . import main_residual as _res

get_deep_feature = _res.get_deep_feature      # same body in both reference files (:81-113 here, :83-115 there)


def process_video_feature(video_feature, network_name):
    """list of per-frame activations -> [T, 2048] (resnet50), [T, 4096] (vgg16) or [T, 3*dim] (vit: token mean | max | std)."""
    rows = []
    for frame in video_feature:
        if network_name == "vit":
            pooled = getattr(frame, "pooled", None)
            rows.append(pooled if pooled is not None else _res.token_stats(frame))
        else:
            rows.append(np.asarray(_res.squeezed(frame)))
    return np.array(rows)
