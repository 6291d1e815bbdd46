#!/usr/bin/env python3
"""Host-side enqueue time of one ResNet-50 forward (GPU box only): the wall time of `eng.resnet50_features` on N fragments with no
synchronisation inside the timed window and one after it - where per-call host work (the schedule is planned on every call) would show.
  RELAX_HIP_LIB=... python tools/resnet_enqueue.py [N=32] [CALLS=200]      prints the median / min / max in microseconds as one JSON line"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import relax_vqa_amd  # noqa: E402,F401
from relax_vqa_amd import synth  # noqa: E402
from relax_vqa_amd.engine import RelaxEngine  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 32
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 200
eng = RelaxEngine(0)
eng.load_resnet50(synth.resnet50_state_dict())
frags = torch.randint(0, 256, (n, 224, 224, 3), dtype=torch.uint8, device="cuda")
for _ in range(20):
    eng.resnet50_features(frags)
torch.cuda.synchronize()
us = []
for _ in range(calls):
    t0 = time.perf_counter()
    eng.resnet50_features(frags)
    us.append((time.perf_counter() - t0) * 1e6)
    torch.cuda.synchronize()
print(json.dumps({"fragments": n, "calls": calls, "enqueue_us_median": round(statistics.median(us), 2), "enqueue_us_min": round(min(us), 2),
                  "enqueue_us_max": round(max(us), 2)}))
