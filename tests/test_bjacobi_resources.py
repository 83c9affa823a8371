"""The kernels of the point-block Jacobi preconditioner (bjacobi_kernels.hpp) keep their budget, read from the compiler's resource
remarks for gfx950 alone: every instantiation of the apply (two types x eight block sizes x three modes) and of the setup is
present, no apply kernel uses scratch or LDS, and VGPRs and occupancy are pinned at the shipped values (8 waves per
SIMD as the conjugate-gradient kernels, except 7 for b = 7 and 8 and for b = 6 in floats, and 6 or 7 for b = 7 in floats, where
the inverse's b groups and two blocks of r exceed 64 registers).  The setup is one-time code: its LDS is the [B | I] image of one
block, its registers are reported, not gated.  (That no sum is contracted into a fused multiply-add is held by the bit-for-bit
tests on the GPU, not here.)  Needs hipcc, not a GPU."""
import os
import re
import shutil
import subprocess

import pytest

from spmv_amd.capi import bjacobi_apply, bjacobi_setup  # noqa: F401  (the entry points that launch these kernels)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spmv-cache-trace_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

SRC = '#include "bjacobi_kernels.hpp"\n' \
      "#define APPLY(T, B, M) template __global__ void spmv::bjacobi_apply_kernel<T, B, M>(long long, const T *, const T *, T *, spmv::v2d *)\n" \
      + "".join("APPLY(%s, %d, %d);\n" % (t, b, m) for t in ("double", "float") for b in range(1, 9) for m in range(3)) \
      + "".join("template __global__ void spmv::bjacobi_setup_kernel<%s>(int, const int *, const int *, const double *, %s *, int *);\n" % (t, t)
                for t in ("double", "float"))
# (type, b): (VGPRs, waves per SIMD) of the modes 0 (apply), 1 (apply with dots), 2 (apply_add)
SHIPPED = {
    ("d", 1): [(20, 8), (26, 8), (26, 8)],
    ("d", 2): [(22, 8), (28, 8), (28, 8)],
    ("d", 3): [(38, 8), (54, 8), (42, 8)],
    ("d", 4): [(34, 8), (44, 8), (38, 8)],
    ("d", 5): [(54, 8), (60, 8), (58, 8)],
    ("d", 6): [(54, 8), (58, 8), (58, 8)],
    ("d", 7): [(62, 8), (68, 7), (62, 8)],
    ("d", 8): [(60, 8), (64, 8), (60, 8)],
    ("f", 1): [(20, 8), (34, 8), (34, 8)],
    ("f", 2): [(42, 8), (54, 8), (50, 8)],
    ("f", 3): [(50, 8), (64, 8), (58, 8)],
    ("f", 4): [(62, 8), (38, 8), (62, 8)],
    ("f", 5): [(63, 8), (62, 8), (62, 8)],
    ("f", 6): [(64, 8), (66, 7), (71, 7)],
    ("f", 7): [(74, 6), (72, 7), (78, 6)],
    ("f", 8): [(56, 8), (66, 7), (60, 8)],
}
SETUP_LDS = 8 * 16 * 8 + 8  # [B | I] of the largest block, and the singular flag


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("bjacobi_resources")
    src = d / "bjacobi.hip"
    src.write_text(SRC)
    # the Makefile's flags
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", str(src), "-o", str(d / "bjacobi.s")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    return r.stdout


def _remarks_of(remarks, mangled):
    m = re.search(r"Function Name: (_ZN4spmv\d+" + re.escape(mangled) + r"\S*)(.*?)(?=Function Name:|\Z)", remarks, re.S)
    assert m, mangled + " not among the remarks"

    def remark(name):
        v = re.search(re.escape(name) + r":\s*(\d+)", m.group(2))
        assert v, name
        return int(v.group(1))

    return remark


def test_forty_eight_apply_kernels():
    assert len(SHIPPED) == 16 and all(len(v) == 3 for v in SHIPPED.values())


@pytest.mark.parametrize("t,b", sorted(SHIPPED))
def test_no_scratch_no_lds_and_the_shipped_registers_in_the_apply(remarks, t, b):
    for mode, (vgprs, waves) in enumerate(SHIPPED[(t, b)]):
        remark = _remarks_of(remarks, "bjacobi_apply_kernelI%sLi%dELi%dE" % (t, b, mode))
        print("%s, b %d, mode %d: %d VGPRs, %d SGPRs, %d bytes of LDS, %d bytes of scratch, occupancy %d" % (
            t, b, mode, remark(" VGPRs"), remark("TotalSGPRs"), remark("LDS Size [bytes/block]"), remark("ScratchSize [bytes/lane]"),
            remark("Occupancy [waves/SIMD]")))
        assert remark("ScratchSize [bytes/lane]") == 0
        assert remark("LDS Size [bytes/block]") == 0
        assert remark(" VGPRs") == vgprs
        assert remark("Occupancy [waves/SIMD]") == waves


@pytest.mark.parametrize("t", ["d", "f"])
def test_the_setup_is_present_and_its_lds_is_one_block(remarks, t):
    remark = _remarks_of(remarks, "bjacobi_setup_kernelI%sE" % t)
    print("setup, %s: %d VGPRs, %d SGPRs, %d bytes of LDS, %d bytes of scratch, occupancy %d" % (
        t, remark(" VGPRs"), remark("TotalSGPRs"), remark("LDS Size [bytes/block]"), remark("ScratchSize [bytes/lane]"),
        remark("Occupancy [waves/SIMD]")))
    assert remark("LDS Size [bytes/block]") == SETUP_LDS and remark("ScratchSize [bytes/lane]") == 0
