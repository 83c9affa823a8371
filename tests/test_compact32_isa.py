"""csr_compact_f32xy_kernel is the tile of the compact kernels (csr_f32values.hpp: f32_tile; csr_compact.hpp: compact_wave) with
float x and y.  What that must not cost, read from the compiler's resource remarks for gfx950 on its two instantiations: no
scratch, at most 64 VGPRs and so 8 waves per SIMD, and exactly the LDS of csr_compact_kernel -- four slices of 516 DOUBLES (the
products stay fp64) and four tables of 8 window bases.  Needs hipcc, not a GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spmv-cache-trace_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

SRC = """#include "csr_compact.hpp"
#define C32(X32) template __global__ void spmv::csr_compact_f32xy_kernel<X32>(int, const int4 *, const int *, const uint16_t *, \\
                                                                              const int32_t *, const int32_t *, const float *, const float *, float *, int)
C32(true);
C32(false);
"""
LDS = 4 * 516 * 8 + 4 * 8 * 4  # 4 waves x ((512 + 4) doubles + 8 bases)
KERNELS = ["csr_compact_f32xy_kernelILb1E", "csr_compact_f32xy_kernelILb0E"]


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("compact32_isa")
    src = d / "compact32.hip"
    src.write_text(SRC)
    # the Makefile's flags
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", str(src), "-o", str(d / "compact32.s")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    return r.stdout


@pytest.mark.parametrize("kernel", KERNELS)
def test_registers_lds_and_occupancy(remarks, kernel):
    # a kernel's remarks: from its "Function Name" line to the next one
    m = re.search(r"Function Name: _ZN4spmv\d+" + kernel + r"(.*?)(?=Function Name:|\Z)", remarks, re.S)
    assert m, kernel + " not among the remarks"

    def remark(name):
        v = re.search(re.escape(name) + r":\s*(\d+)", m.group(1))
        assert v, name
        return int(v.group(1))

    print("%s: %d VGPRs, %d SGPRs, %d bytes of LDS" % (kernel, remark(" VGPRs"), remark("TotalSGPRs"), remark("LDS Size [bytes/block]")))
    assert remark("ScratchSize [bytes/lane]") == 0
    assert remark("Occupancy [waves/SIMD]") == 8
    assert remark(" VGPRs") <= 64  # the budget of 8 waves per SIMD
    assert remark("LDS Size [bytes/block]") == LDS == 16640
