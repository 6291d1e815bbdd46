"""The ResNet-50 block schedule is host logic (csrc/host_logic.cpp: rn_plan): which of the six launch forms each bottleneck runs, the form
every tensor travels in, the per-image slots.  Checked here without a GPU, over every option combination and request form."""
import ctypes as C
import os
import subprocess

import pytest

from tests import rn_schedule_checks as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    """csrc/host_logic.cpp alone with its test entry points, built into a temporary directory (plain g++, no HIP)."""
    out = tmp_path_factory.mktemp("host") / "libhost.so"
    src = os.path.join(ROOT, "relax-vqa_amd", "csrc", "host_logic.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-DRELAX_HOST_TEST_API", src, "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    lib.relax_host_rn_plan.restype = C.c_int
    return lib


def test_every_option_combination_and_request(host_lib):
    """32 switch settings x "gemm_precision" 2 / 3 x 5 requests: slot budget (and the refusal one slot short of it), dataflow, fp32 copies exactly
    where something reads them, write-before-read of every slot, request-independence of the launch forms and of no_split."""
    assert rc.check_all(host_lib) == 320


def test_default_schedules_written_out(host_lib):
    rc.check_default_schedules(host_lib)


def test_over_budget_plan_is_refused_before_anything_runs(host_lib):
    stem, _ = rc.plan(host_lib, (3, 1, 1, 1, 1, 1), rc.REQUESTS["layer stack + pool"])
    assert 0 < stem["n_slots"] <= rc.IMG_SLOTS
    msg = rc.plan(host_lib, (3, 1, 1, 1, 1, 1), rc.REQUESTS["layer stack + pool"], max_slots=8)
    assert msg == "resnet50: %d per-image scale slots used, 8 reserved" % stem["n_slots"]
