"""Writes tests/golden/whole_residual.npz: the pooling of the REFERENCE's own src/main_residual.py and src/main_layer.py
(process_video_feature of each) on recorded-shape activations, as data.

Runs on a CPU host that has the reference checkout (its path: the first argument, or RELAX_REFERENCE).  Imports the two
drivers with cv2, the extractors and the absent third-party modules mocked, the way oracle/make_golden.py imports the
fragment drivers (the numpy functions run unchanged); no reference source is copied.

    python tools/make_whole_residual_golden.py REFERENCE_CHECKOUT

Stored: two frames each of a ResNet-50 avgpool activation [2048,1,1], a VGG-16 fc2 activation [4096] and ViT-tiny patch
tokens [196,192] (seeded; post-ReLU activations are non-negative with exact zeros, tokens are signed), and what the two
reference functions return for them."""
import importlib
import os
import sys
from unittest import mock

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("RELAX_REFERENCE")
if not REF:
    sys.exit("usage: make_whole_residual_golden.py REFERENCE_CHECKOUT (or set RELAX_REFERENCE)")
OUT = os.path.join(ROOT, "tests", "golden", "whole_residual.npz")


def import_reference():
    try:
        importlib.import_module("pandas")
    except Exception:
        sys.modules["pandas"] = mock.MagicMock()
    for m in ["cv2", "extractor", "extractor.visualise_vgg_layer", "extractor.visualise_resnet_layer",
              "extractor.visualise_vit_layer", "video_frames_extract", "utils", "utils.logger_setup"]:
        sys.modules[m] = mock.MagicMock()
    sys.path.insert(0, os.path.join(REF, "src"))
    import main_layer
    import main_residual
    return main_residual, main_layer


def main():
    res, lay = import_reference()
    g = np.random.default_rng(20261017)
    relu = lambda a: np.maximum(a, 0).astype(np.float32)
    acts = {"resnet50": relu(g.normal(0.3, 1.0, (2, 2048, 1, 1))),
            "vgg16": relu(g.normal(-0.2, 1.0, (2, 4096))),
            "vit": g.normal(0.0, 2.0, (2, 196, 192)).astype(np.float32)}
    out = {}
    for name, a in acts.items():
        out[f"act_{name}"] = a
        out[f"residual_{name}"] = np.asarray(res.process_video_feature(list(a), name))
        out[f"layer_{name}"] = np.asarray(lay.process_video_feature(list(a), name))
        print(name, a.shape, out[f"residual_{name}"].shape, out[f"residual_{name}"].dtype, out[f"layer_{name}"].shape)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
