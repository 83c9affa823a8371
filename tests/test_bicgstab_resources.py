"""The kernels of the BiCGStab updates (bicgstab_updates.hpp) keep their budget, read from the compiler's resource remarks for gfx950
alone, for all twelve instantiations -- {s, direction} x {double, float} x {with, without minv} and step x {double, float} x {with,
without shat}: no scratch, no LDS, at most 64 VGPRs and so 8 waves per SIMD.  (That no update is contracted into a fused
multiply-add, and that an absent array is neither loaded nor stored, is held by the bit-for-bit tests and the guard bands on the
GPU, not here.)  Needs hipcc, not a GPU."""
import os
import re
import shutil
import subprocess

import pytest

from spmv_amd.capi import bicgstab_direction, bicgstab_s, bicgstab_step  # noqa: F401  (the entry points that launch these kernels)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spmv-cache-trace_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

SRC = """#include "bicgstab_updates.hpp"
#define S(T, HASM) template __global__ void spmv::bicgstab_s_kernel<T, HASM>(long long, const double *, const double *, const T *, T *, \\
    const T *, T *)
#define STEP(T, HASS) template __global__ void spmv::bicgstab_step_kernel<T, HASS>(long long, const double *, const double *, const double *, \\
    const double *, const T *, const T *, const T *, const T *, T *, T *, spmv::v2d *)
#define DIRECTION(T, HASM) template __global__ void spmv::bicgstab_direction_kernel<T, HASM>(long long, const double *, const double *, \\
    const double *, const double *, const double *, const double *, const T *, const T *, T *, const T *, T *)
S(double, true); S(double, false); S(float, true); S(float, false);
STEP(double, true); STEP(double, false); STEP(float, true); STEP(float, false);
DIRECTION(double, true); DIRECTION(double, false); DIRECTION(float, true); DIRECTION(float, false);
"""
KERNELS = ["%sI%sLb%dE" % (name, t, flag) for name in ("bicgstab_s_kernel", "bicgstab_step_kernel", "bicgstab_direction_kernel") for t in "df"
           for flag in (1, 0)]


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("bicgstab_resources")
    src = d / "bicgstab.hip"
    src.write_text(SRC)
    # the Makefile's flags
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", str(src), "-o", str(d / "bicgstab.s")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    return r.stdout


def test_twelve_instantiations():
    assert len(set(KERNELS)) == 12


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_no_scratch_no_lds_at_most_64_vgprs_and_8_waves_per_simd(remarks, kernel):
    # a kernel's remarks: from its "Function Name" line to the next one
    m = re.search(r"Function Name: (_ZN4spmv\d+" + kernel + r"\S*)(.*?)(?=Function Name:|\Z)", remarks, re.S)
    assert m, kernel + " not among the remarks"

    def remark(name):
        v = re.search(re.escape(name) + r":\s*(\d+)", m.group(2))
        assert v, name
        return int(v.group(1))

    print("%s: %d VGPRs, %d SGPRs, %d bytes of LDS, %d bytes of scratch, occupancy %d" % (
        kernel, remark(" VGPRs"), remark("TotalSGPRs"), remark("LDS Size [bytes/block]"), remark("ScratchSize [bytes/lane]"),
        remark("Occupancy [waves/SIMD]")))
    assert remark("ScratchSize [bytes/lane]") == 0
    assert remark("LDS Size [bytes/block]") == 0
    assert remark(" VGPRs") <= 64  # the budget of 8 waves per SIMD
    assert remark("Occupancy [waves/SIMD]") == 8
