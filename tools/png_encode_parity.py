"""Measures the size of the encoder's streams (host build of csrc/png_deflate.h, the device's bytes) against zlib's Z_RLE at
level 6 over the same filtered bytes, for the golden-frame crops and the gradients of the test corpus, and writes
profiles/png_encode_parity.json: the worst ratio is what tests/test_png_encode_cpu.py gates on (plus 5 %).  No GPU needed."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import png_encode_driver as drv  # noqa: E402


def main():
    ratios = drv.size_parity()
    worst = max(ratios, key=ratios.get)
    big = {k: v for k, v in ratios.items() if "224x224" in k or "x1920" in k}
    res = dict(yardstick="zlib.compressobj(6, DEFLATED, 15, 9, Z_RLE) over the encoder's filtered bytes",
               worst_ratio=round(ratios[worst], 4), worst_case=worst,
               worst_ratio_224x224_and_wider=round(max(big.values()), 4), cases=len(ratios),
               ratios={k: round(v, 4) for k, v in sorted(ratios.items())})
    path = os.path.join(ROOT, "profiles", "png_encode_parity.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("worst_ratio", "worst_case", "worst_ratio_224x224_and_wider", "cases")}))


if __name__ == "__main__":
    main()
