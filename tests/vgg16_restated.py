"""VGG-16 restated from the published architecture (torchvision `vgg16`, configuration D, no BatchNorm) as the parity oracle of
the VGG-16 backbone: torchvision is not a dependency of the project.  A real nn.Sequential with torchvision's module indices and
ReLU(inplace=True), read through forward hooks as src/extractor/visualise_vgg.py / visualise_vgg_layer.py read it - so the taps
are post-ReLU by construction (the in-place ReLU behind each hooked module rectifies the tensor the hook holds)."""
import numpy as np
import torch
from torch import nn

from oracle.resnet50_ref import preprocess_bgr_u8  # noqa: F401  (ToTensor + Normalize of a BGR fragment: the same front-end)

CFG_D = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"]
CONV_INDEX = [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]
TAP_SHAPES = [(64, 224)] * 2 + [(128, 112)] * 2 + [(256, 56)] * 3 + [(512, 28)] * 3 + [(512, 14)] * 3
LAYER_STACK_DIM = sum(c for c, _ in TAP_SHAPES)     # 4224
POOL_DIM = 4096 + 3                                  # 4099


class VGG16(nn.Module):
    def __init__(self):
        super().__init__()
        layers, cin = [], 3
        for v in CFG_D:
            if v == "M":
                layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            else:
                layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
                cin = v
        self.features = nn.Sequential(*layers)
        self.avgpool = nn.AdaptiveAvgPool2d((7, 7))
        self.classifier = nn.Sequential(nn.Linear(512 * 7 * 7, 4096), nn.ReLU(True), nn.Dropout(),
                                        nn.Linear(4096, 4096), nn.ReLU(True), nn.Dropout(), nn.Linear(4096, 1000))

    def forward(self, x):
        x = self.avgpool(self.features(x))
        return self.classifier(torch.flatten(x, 1))


def build(state_dict, dtype=torch.float32):
    """The restated net with the given torchvision-keyed weights (classifier.6 may be absent: it is zero then; nothing reads it)."""
    m = VGG16()
    sd = {k: torch.as_tensor(np.asarray(v)) for k, v in state_dict.items()}
    full = m.state_dict()
    for k in full:
        if k not in sd:
            assert k.startswith("classifier.6."), k
            sd[k] = torch.zeros_like(full[k])
    m.load_state_dict(sd)
    return m.to(dtype).eval()


def hooked(model, x, modules):
    """One forward with a hook on each module; the hooked tensors are read after the forward, as the reference's `.cpu()` does."""
    acts, handles = [], []
    for mod in modules:
        handles.append(mod.register_forward_hook(lambda _m, _i, out: acts.append(out)))
    with torch.no_grad():
        model(x)
    for hd in handles:
        hd.remove()
    return acts


def taps(model, x):
    """-> 15 tensors: features[CONV_INDEX] [N,C,H,W], classifier[0] (fc1) and classifier[3] (fc2) [N,4096] - all post-ReLU."""
    mods = [model.features[i] for i in CONV_INDEX] + [model.classifier[0], model.classifier[3]]
    return hooked(model, x, mods)


def features(tap_list):
    """process_video_feature: layer stack = per-tap spatial means [N,4224]; pool = fc2 | mean | max | population std [N,4099]."""
    ls = torch.cat([t.mean(dim=(2, 3)) for t in tap_list[:13]], dim=1)
    f = tap_list[14]
    pool = torch.cat([f, f.mean(1, keepdim=True), f.max(1, keepdim=True).values, f.std(1, unbiased=False, keepdim=True)], dim=1)
    return ls, pool
