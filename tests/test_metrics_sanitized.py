"""CPU sanitizer pass on the metrics core: csrc/metrics_core.h - the pair counting, the rank finish, the logistic model, the
damped 4x4 solve and the Levenberg-Marquardt step rule the gfx950 kernels run - built as one thread of host code alone with
-fsanitize=address,undefined (make sanitize_metrics) and driven by tests/metrics_driver.py in a subprocess that preloads
libasan, over the rank cases and the well- and ill-conditioned fit cases of tests/metrics_cases.py and a non-finite input,
with exactly sized heap buffers: no sanitizer report.  Never on the GPU."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "relax-vqa_amd", "csrc")


def _gcc_file(name):
    out = subprocess.run(["gcc", f"-print-file-name={name}"], capture_output=True, text=True).stdout.strip()
    return out if os.path.isabs(out) and os.path.exists(out) else None


def test_metrics_core_under_asan_and_ubsan():
    asan, ubsan = _gcc_file("libasan.so"), _gcc_file("libubsan.so")
    if not asan:
        pytest.skip("no libasan in this toolchain")
    subprocess.run(["make", "-C", CSRC, "sanitize_metrics"], check=True, capture_output=True)
    env = dict(os.environ, LD_PRELOAD=":".join(p for p in (asan, ubsan) if p),
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
               PYTHONDONTWRITEBYTECODE="1")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "metrics_driver.py")], env=env, capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
    assert "METRICS_SANITIZED_OK" in res.stdout
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-4000:]
