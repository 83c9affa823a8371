"""The kernels of the scaled multiplies with dots (csr_dots.hpp, csr_compact.hpp: the family's tile with a third epilogue and a
wave reduction behind it) keep the family's budget, read from the compiler's resource remarks and assembly for gfx950 for every
instantiation -- four kernels x BETA0 x with / without w; there are no X32 = false ones (include/spmv_hip_dots.h): no scratch, at
most 64 VGPRs and so 8 waves per SIMD, the LDS of the sibling kernel exactly (four slices of 516 doubles, plus four tables of 8
window bases in the compact kernels only: the wave reduction and the slot take none), and no fused multiply-add in fp64 anywhere:
the products of the dots are rounded before they are added.  Needs hipcc, not a GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spmv-cache-trace_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

SRC = """#include "csr_compact.hpp"
#define F32(BETA0, HASW) template __global__ void spmv::csr_f32values_scaled_dots_kernel<BETA0, HASW>(int, const int4 *, const int32_t *, \\
    const int32_t *, const float *, const double *, double, double, const double *, double *, const double *, spmv::v2d *, int)
#define C16(NAME, V, T, BETA0, HASW) template __global__ void spmv::NAME<BETA0, HASW>(int, const int4 *, const int *, const uint16_t *, \\
    const int32_t *, const int32_t *, const V *, const T *, double, double, const T *, T *, const T *, spmv::v2d *, int)
#define ALL(M, ...) M(__VA_ARGS__, true, true); M(__VA_ARGS__, true, false); M(__VA_ARGS__, false, true); M(__VA_ARGS__, false, false)
F32(true, true); F32(true, false); F32(false, true); F32(false, false);
ALL(C16, csr_compact_scaled_dots_kernel, float, double);
ALL(C16, csr_compact_f64_scaled_dots_kernel, double, double);
ALL(C16, csr_compact_f32xy_scaled_dots_kernel, float, float);
"""
SLICES = 4 * 516 * 8  # 4 waves x (512 + 4) doubles
TABLES = 4 * 8 * 4    # 4 waves x 8 window bases
FAMILIES = {"csr_f32values_scaled_dots_kernel": SLICES, "csr_compact_scaled_dots_kernel": SLICES + TABLES,
            "csr_compact_f64_scaled_dots_kernel": SLICES + TABLES, "csr_compact_f32xy_scaled_dots_kernel": SLICES + TABLES}
KERNELS = {"%sILb%dELb%dE" % (name, beta0, hasw): lds for name, lds in FAMILIES.items() for beta0 in (1, 0) for hasw in (1, 0)}


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("dots_isa")
    src = d / "dots.hip"
    src.write_text(SRC)
    # the Makefile's flags
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", str(src), "-o", str(d / "dots.s")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    return r.stdout, (d / "dots.s").read_text()


def test_sixteen_instantiations():
    assert len(KERNELS) == 16


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_registers_lds_occupancy_and_no_fused_multiply_add(compiled, kernel):
    remarks, asm = compiled
    # a kernel's remarks: from its "Function Name" line to the next one
    m = re.search(r"Function Name: (_ZN4spmv\d+" + kernel + r"\S*)(.*?)(?=Function Name:|\Z)", remarks, re.S)
    assert m, kernel + " not among the remarks"

    def remark(name):
        v = re.search(re.escape(name) + r":\s*(\d+)", m.group(2))
        assert v, name
        return int(v.group(1))

    print("%s: %d VGPRs, %d SGPRs, %d bytes of LDS" % (kernel, remark(" VGPRs"), remark("TotalSGPRs"), remark("LDS Size [bytes/block]")))
    assert remark("ScratchSize [bytes/lane]") == 0
    assert remark("Occupancy [waves/SIMD]") == 8
    assert remark(" VGPRs") <= 64  # the budget of 8 waves per SIMD
    assert remark("LDS Size [bytes/block]") == KERNELS[kernel]
    # the kernel's instructions: from its label to the end of the function
    symbol = m.group(1)
    body = re.search(r"^" + re.escape(symbol) + r":[^\n]*\n(.*?)^\.Lfunc_end", asm, re.S | re.M)
    assert body, symbol + " not in the assembly"
    text = body.group(1)
    assert "v_mul_f64" in text and "v_add_f64" in text
    assert not re.search(r"v_fma(c|ak|mk)?_f64|v_pk_fma", text), kernel + ": a fused multiply-add"
    # both dots leave the wave as ONE 16-byte vector store (the row stores are 8 or 4 bytes wide)
    assert len(re.findall(r"global_store_dwordx4", text)) == 1
