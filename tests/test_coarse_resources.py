"""The kernels of include/spmv_hip_coarse.h (coarse_kernels.hpp) keep their budget, read from the compiler's resource remarks for
gfx950 with the Makefile's flags alone: the apply in both types uses no scratch and no LDS and runs at 8 waves per SIMD, with its
VGPRs pinned at the shipped values (four elements of a lane in flight), and multiplies and adds without a fused instruction.  The
kernels of the set-up are one-time code: no scratch, otherwise reported, not gated.  Needs hipcc, not a GPU."""
import os
import re
import shutil
import subprocess

import pytest

from spmv_amd.capi import coarse_apply, coarse_setup  # noqa: F401  (the entry points that launch these kernels)
from test_agg_resources import _remarks_of, _report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spmv-cache-trace_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

SRC = '#include "coarse_kernels.hpp"\n' \
      + "".join("template __global__ void spmv::coarse_apply_kernel<%s>(int, int, const %s *, const %s *, %s *);\n" % (t, t, t, t)
                + "template __global__ void spmv::coarse_store_kernel<%s>(int, int, const double *, const int *, %s *);\n" % (t, t)
                for t in ("double", "float"))
# type: VGPRs (at 8 waves per SIMD)
SHIPPED = {"d": 28, "f": 28}
ONE_TIME = ("coarse_init_kernel", "coarse_densify_kernel", "coarse_pivot_kernel", "coarse_update_kernel", "coarse_store_kernelIdE",
            "coarse_store_kernelIfE")


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("coarse_resources")
    src = d / "coarse.hip"
    src.write_text(SRC)
    # the Makefile's flags
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", str(src), "-o", str(d / "coarse.s")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    return r.stdout, (d / "coarse.s").read_text()


@pytest.mark.parametrize("t", ["d", "f"])
def test_no_scratch_no_lds_eight_waves_and_the_shipped_registers_in_the_apply(remarks, t):
    remark = _remarks_of(remarks[0], "coarse_apply_kernelI%sE" % t)
    _report("apply, %s" % t, remark)
    assert remark("ScratchSize [bytes/lane]") == 0
    assert remark("LDS Size [bytes/block]") == 0
    assert remark("Occupancy [waves/SIMD]") == 8
    assert remark(" VGPRs") == SHIPPED[t]


def test_the_apply_and_the_update_round_every_product_on_its_own(remarks):
    """No fused multiply-add in the apply or in the update of the other rows (the pivot kernel's division is the compiler's own
    sequence, which does use them), and no atomic in the apply."""
    for name in ("coarse_apply_kernelIdE", "coarse_apply_kernelIfE", "coarse_update_kernel"):
        m = re.search(r"^(_ZN4spmv\d+%s\w*):[^\n]*\n(.*?)\n\.Lfunc_end" % name, remarks[1], re.S | re.M)
        assert m, name
        assert not re.findall(r"v_fma\w*_f64|v_fmac_f64|atomic", m.group(2)), name
        assert len(re.findall(r"v_mul_f64", m.group(2))) >= 1, name


def test_the_one_time_kernels_use_no_scratch_and_are_reported(remarks):
    for name in ONE_TIME:
        remark = _remarks_of(remarks[0], name)
        _report(name, remark)
        assert remark("ScratchSize [bytes/lane]") == 0
