"""The scaled kernels (csr_f32values.hpp, csr_compact.hpp: the family's tile with another epilogue) keep the family's budget, read
from the compiler's resource remarks for gfx950 for every instantiation -- X32 true and false (x of 4 GiB and more: compiled and
checked here, never run), BETA0 true and false: no scratch, at most 64 VGPRs and so 8 waves per SIMD, and the LDS of the sibling
kernel exactly: four slices of 516 doubles, plus four tables of 8 window bases in the compact kernels only.  Resource remarks only.
Needs hipcc, not a GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spmv-cache-trace_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

SRC = """#include "csr_compact.hpp"
#define F32(X32, BETA0) template __global__ void spmv::csr_f32values_scaled_kernel<X32, BETA0>(int, const int4 *, const int32_t *, const int32_t *, \\
    const float *, const double *, double, double, const double *, double *, int)
#define C16(NAME, V, T, X32, BETA0) template __global__ void spmv::NAME<X32, BETA0>(int, const int4 *, const int *, const uint16_t *, \\
    const int32_t *, const int32_t *, const V *, const T *, double, double, const T *, T *, int)
#define ALL(M, ...) M(__VA_ARGS__, true, true); M(__VA_ARGS__, true, false); M(__VA_ARGS__, false, true); M(__VA_ARGS__, false, false)
F32(true, true); F32(true, false); F32(false, true); F32(false, false);
ALL(C16, csr_compact_scaled_kernel, float, double);
ALL(C16, csr_compact_f64_scaled_kernel, double, double);
ALL(C16, csr_compact_f32xy_scaled_kernel, float, float);
"""
SLICES = 4 * 516 * 8  # 4 waves x (512 + 4) doubles
TABLES = 4 * 8 * 4    # 4 waves x 8 window bases
FAMILIES = {"csr_f32values_scaled_kernel": SLICES, "csr_compact_scaled_kernel": SLICES + TABLES,
            "csr_compact_f64_scaled_kernel": SLICES + TABLES, "csr_compact_f32xy_scaled_kernel": SLICES + TABLES}
KERNELS = {"%sILb%dELb%dE" % (name, x32, beta0): lds for name, lds in FAMILIES.items() for x32 in (1, 0) for beta0 in (1, 0)}


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("scaled_isa")
    src = d / "scaled.hip"
    src.write_text(SRC)
    # the Makefile's flags
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", str(src), "-o", str(d / "scaled.s")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    return r.stdout


def test_sixteen_instantiations():
    assert len(KERNELS) == 16


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
