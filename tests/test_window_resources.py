"""The kernels of the symmetric and the transposed multiply (csr_symmetric.hpp, csr_transpose.hpp over window_walk.hpp) keep their
budget, read from the compiler's resource remarks for gfx950 with the Makefile's flags alone: all eight instantiations are
present, none uses scratch or static LDS (the windows are dynamic LDS, up to 80 KB per workgroup), each runs at 8 waves per SIMD
and with the VGPRs it ships with.  The launch bound of 512 threads x 2 workgroups per CU asks for 4 waves per SIMD only, which
128 VGPRs would allow; the bound here is the 64 that 8 waves take, because that is what the kernels had before the two walks
became one.  Needs hipcc, not a GPU."""
import os
import re
import shutil
import subprocess

import pytest

from spmv_amd.capi import SymPlan, TrPlan  # noqa: F401  (the plans that launch these kernels)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spmv-cache-trace_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

SYM_ARGS = "(int, int, const int *, const int *, const double *, const double *, double *, const int2 *, int, int, double)"
TR_ARGS = "(int, int, int, const int *, const int *, const double *, const double *, double *, const int2 *, int, int)"
# (kernel, KW): VGPRs
SHIPPED = {
    ("csr_symv_kernel", 0): 56, ("csr_symv_kernel", 1): 56, ("csr_symv_kernel", 3): 56, ("csr_symv_kernel", 7): 58,
    ("csr_spmv_t_kernel", 1): 55, ("csr_spmv_t_kernel", 2): 55, ("csr_spmv_t_kernel", 4): 55, ("csr_spmv_t_kernel", 8): 51,
}
SRC = '#include "csr_symmetric.hpp"\n#include "csr_transpose.hpp"\n' \
      + "".join("template __global__ void spmv::%s<%d>%s;\n" % (k, kw, SYM_ARGS if k == "csr_symv_kernel" else TR_ARGS) for k, kw in sorted(SHIPPED))


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("window_resources")
    src = d / "window.hip"
    src.write_text(SRC)
    # the Makefile's flags
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", str(src), "-o", str(d / "window.s")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    return r.stdout


@pytest.mark.parametrize("kernel, kw", sorted(SHIPPED))
def test_no_scratch_no_static_lds_eight_waves_and_the_shipped_registers(remarks, kernel, kw):
    m = re.search(r"Function Name: (_ZN4spmv\d+%sILi%dEE\S*)(.*?)(?=Function Name:|\Z)" % (kernel, kw), remarks, re.S)
    assert m, "%s<%d> not among the remarks" % (kernel, kw)

    def remark(name):
        v = re.search(re.escape(name) + r":\s*(\d+)", m.group(2))
        assert v, name
        return int(v.group(1))

    print("%s<%d>: %d VGPRs, %d SGPRs, %d bytes of static LDS, %d bytes of scratch, occupancy %d" % (
        kernel, kw, remark(" VGPRs"), remark("TotalSGPRs"), remark("LDS Size [bytes/block]"), remark("ScratchSize [bytes/lane]"),
        remark("Occupancy [waves/SIMD]")))
    assert remark("ScratchSize [bytes/lane]") == 0
    assert remark("LDS Size [bytes/block]") == 0
    assert remark("Occupancy [waves/SIMD]") == 8
    assert SHIPPED[kernel, kw] <= 64
    assert remark(" VGPRs") == SHIPPED[kernel, kw]
