"""The two kernels that make a compact plan from device columns (c16_plan_kernels.hpp, behind include/spmv_hip_compact_device.h)
keep their budget, read from the compiler's resource remarks for gfx950 with the Makefile's flags alone: no scratch -- the eight
columns of a lane and the eight bases of a tile stay in registers.  They are set-up code: VGPRs, LDS and occupancy are reported,
not gated.  Needs hipcc, not a GPU."""
import os
import shutil
import subprocess

import pytest

from spmv_amd.capi import C16Plan  # noqa: F401  (from_device is the entry point that launches these kernels)
from test_agg_resources import _remarks_of, _report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spmv-cache-trace_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

SRC = '#include "c16_plan_kernels.hpp"\n'
KERNELS = ("c16_windows_kernel", "c16_codes_kernel")


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    assert callable(C16Plan.from_device)
    if HIPCC is None:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("c16_plan_resources")
    src = d / "c16_plan.hip"
    src.write_text(SRC)
    # the Makefile's flags
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", str(src), "-o", str(d / "c16_plan.s")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    return r.stdout


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_and_the_rest_reported(remarks, kernel):
    remark = _remarks_of(remarks, kernel)
    _report(kernel, remark)
    assert remark("ScratchSize [bytes/lane]") == 0
