"""The two fp32-value kernels share one tile (csr_f32values.hpp: f32_tile) and differ in their column source.  What that must
not cost, read from the compiler's resource remarks for gfx950: no scratch, at most 64 VGPRs and so 8 waves per SIMD, and the LDS
of each kernel exactly -- four slices of 516 doubles, plus, in csr_compact_kernel ONLY, four tables of 8 window bases (the
fp32-value kernel has not acquired the code path's table).  Needs hipcc, not a GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spmv-cache-trace_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

SRC = """#include "csr_compact.hpp"
#define F32(X32) template __global__ void spmv::csr_f32values_kernel<X32>(int, const int4 *, const int32_t *, const int32_t *, \\
                                                                          const float *, const double *, double *, int)
#define C16(X32) template __global__ void spmv::csr_compact_kernel<X32>(int, const int4 *, const int *, const uint16_t *, \\
                                                                        const int32_t *, const int32_t *, const float *, const double *, double *, int)
F32(true);
F32(false);
C16(true);
C16(false);
"""
SLICES = 4 * 516 * 8  # 4 waves x (512 + 4) doubles
KERNELS = {"csr_f32values_kernelILb1E": SLICES, "csr_f32values_kernelILb0E": SLICES,
           "csr_compact_kernelILb1E": SLICES + 4 * 8 * 4, "csr_compact_kernelILb0E": SLICES + 4 * 8 * 4}


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("f32_family_isa")
    src = d / "f32_family.hip"
    src.write_text(SRC)
    # the Makefile's flags
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", str(src), "-o", str(d / "f32_family.s")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    return r.stdout


@pytest.mark.parametrize("kernel", sorted(KERNELS))
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
    assert remark("LDS Size [bytes/block]") == KERNELS[kernel]
