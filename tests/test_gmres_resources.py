"""The kernels of the GMRES updates (gmres_updates.hpp) keep their budget, read from the compiler's resource remarks for gfx950
alone: every instantiation is present, none uses scratch, the streaming kernels -- project, axpys (update and the two
corrections) and scale -- use no LDS, and VGPRs and occupancy are pinned at the shipped values (project trades
occupancy for register blocks of up to eight vectors, the update and the corrections for a lane's whole share of a chunk with two
vectors in flight; scale and the small kernels keep 8 waves per SIMD).  (That no update is contracted into
a fused multiply-add and that a sum does not depend on the register block is held by the bit-for-bit tests on the GPU, not here.)
Needs hipcc, not a GPU."""
import os
import re
import shutil
import subprocess

import pytest

from spmv_amd.capi import gmres_project, gmres_update  # noqa: F401  (the entry points that launch these kernels)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spmv-cache-trace_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

SRC = """#include "gmres_updates.hpp"
#define PROJECT(T) template __global__ void spmv::gmres_project_kernel<T>(long long, int, const T *, long long, const T *, double *, long long)
#define AXPYS(T, MODE) template __global__ void spmv::gmres_axpys_kernel<T, MODE>(long long, int, const T *, long long, const double *, T *, \\
    const T *, spmv::v2d *)
#define SCALE(T, HASM) template __global__ void spmv::gmres_scale_kernel<T, HASM>(long long, const double *, T *, const T *, T *)
PROJECT(double); PROJECT(float);
AXPYS(double, 0); AXPYS(double, 1); AXPYS(double, 2); AXPYS(float, 0); AXPYS(float, 1); AXPYS(float, 2);
SCALE(double, true); SCALE(double, false); SCALE(float, true); SCALE(float, false);
template __global__ void spmv::gmres_reduce_kernel<256>(int, int, spmv::v2d *, long long, long long, long long, double *, int);
"""
# kernel: (VGPRs, waves per SIMD, streaming)
SHIPPED = {
    "gmres_project_kernelId": (100, 4, True), "gmres_project_kernelIf": (92, 5, True),
    "gmres_axpys_kernelIdLi0E": (98, 4, True), "gmres_axpys_kernelIdLi1E": (82, 5, True), "gmres_axpys_kernelIdLi2E": (84, 5, True),
    "gmres_axpys_kernelIfLi0E": (104, 4, True), "gmres_axpys_kernelIfLi1E": (78, 6, True), "gmres_axpys_kernelIfLi2E": (98, 4, True),
    "gmres_scale_kernelIdLb1E": (24, 8, True), "gmres_scale_kernelIdLb0E": (24, 8, True),
    "gmres_scale_kernelIfLb1E": (36, 8, True), "gmres_scale_kernelIfLb0E": (54, 8, True),
    "gmres_reduce_kernelILi256E": (16, 8, False), "gmres_start_kernelE": (12, 8, False), "gmres_column_kernelE": (39, 8, False),
    "gmres_solve_kernelE": (12, 8, False),
}


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("gmres_resources")
    src = d / "gmres.hip"
    src.write_text(SRC)
    # the Makefile's flags
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", str(src), "-o", str(d / "gmres.s")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    return r.stdout


def test_sixteen_kernels():
    assert len(SHIPPED) == 16 and sum(1 for v in SHIPPED.values() if v[2]) == 12


@pytest.mark.parametrize("kernel", sorted(SHIPPED))
def test_no_scratch_no_lds_in_the_streaming_kernels_and_the_shipped_registers(remarks, kernel):
    # a kernel's remarks: from its "Function Name" line to the next one
    m = re.search(r"Function Name: (_ZN4spmv\d+" + kernel + r"\S*)(.*?)(?=Function Name:|\Z)", remarks, re.S)
    assert m, kernel + " not among the remarks"

    def remark(name):
        v = re.search(re.escape(name) + r":\s*(\d+)", m.group(2))
        assert v, name
        return int(v.group(1))

    vgprs, waves, streaming = SHIPPED[kernel]
    print("%s: %d VGPRs, %d SGPRs, %d bytes of LDS, %d bytes of scratch, occupancy %d" % (
        kernel, remark(" VGPRs"), remark("TotalSGPRs"), remark("LDS Size [bytes/block]"), remark("ScratchSize [bytes/lane]"),
        remark("Occupancy [waves/SIMD]")))
    assert remark("ScratchSize [bytes/lane]") == 0
    if streaming:
        assert remark("LDS Size [bytes/block]") == 0
    assert remark(" VGPRs") == vgprs
    assert remark("Occupancy [waves/SIMD]") == waves
