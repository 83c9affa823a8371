"""The kernels of the conjugate-gradient updates (cg_updates.hpp) keep their budget, read from the compiler's resource remarks and
assembly for gfx950 for all eight instantiations -- {step, direction} x {double, float} x {with, without minv}: no scratch, at
most 64 VGPRs and so 8 waves per SIMD, no LDS, 16-byte loads and stores, fp64 products and sums, no barrier and no atomics.
(That no update is contracted into a fused multiply-add is held by the bit-for-bit tests on the GPU, not here: the IEEE division
of num / den expands into fp64 FMAs.)  Needs hipcc, not a GPU."""
import os
import re
import shutil
import subprocess

import pytest

from spmv_amd.capi import cg_direction, cg_step  # noqa: F401  (the entry points that launch these kernels)

ROOT =os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spmv-cache-trace_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

SRC = """#include "cg_updates.hpp"
#define STEP(T, HASM) template __global__ void spmv::cg_step_kernel<T, HASM>(long long, const double *, const double *, const T *, const T *, \\
    T *, T *, const T *, spmv::v2d *)
#define DIRECTION(T, HASM) template __global__ void spmv::cg_direction_kernel<T, HASM>(long long, const double *, const double *, const T *, \\
    const T *, T *)
STEP(double, true); STEP(double, false); STEP(float, true); STEP(float, false);
DIRECTION(double, true); DIRECTION(double, false); DIRECTION(float, true); DIRECTION(float, false);
"""
KERNELS = ["%sI%sLb%dE" % (name, t, hasm) for name in ("cg_step_kernel", "cg_direction_kernel") for t in "df" for hasm in (1, 0)]


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("krylov_isa")
    src = d / "krylov.hip"
    src.write_text(SRC)
    # the Makefile's flags
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", str(src), "-o", str(d / "krylov.s")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    return r.stdout, (d / "krylov.s").read_text()


def test_eight_instantiations():
    assert len(set(KERNELS)) == 8


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_registers_lds_occupancy_and_vector_width(compiled, kernel):
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
    assert remark("LDS Size [bytes/block]") == 0
    # the kernel's instructions: from its label to the end of the function
    symbol = m.group(1)
    body = re.search(r"^" + re.escape(symbol) + r":[^\n]*\n(.*?)^\.Lfunc_end", asm, re.S | re.M)
    assert body, symbol + " not in the assembly"
    text = body.group(1)
    assert "global_load_dwordx4" in text and "global_store_dwordx4" in text
    assert "v_mul_f64" in text and "v_add_f64" in text
    assert not re.search(r"s_barrier|atomic|ds_read|ds_write|scratch_", text), kernel
