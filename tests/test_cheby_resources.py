"""The kernels of the Chebyshev polynomial preconditioner (cheby_updates.hpp) keep their budget, read from the compiler's resource
remarks for gfx950 with the Makefile's flags alone: every instantiation of the step (two types x minv or none x six modes) is
present, none uses scratch or LDS, and VGPRs and occupancy are pinned at the shipped values (8 waves per SIMD as the
conjugate-gradient kernels, all 24 on the streaming driver).  The bound and the coefficients are one-time code: reported, not
gated.  (That no sum is contracted into a fused multiply-add is held by the bit-for-bit tests on the GPU, not here.)  Needs hipcc,
not a GPU."""
import os
import re
import shutil
import subprocess

import pytest

from spmv_amd.capi import cheby_bound, cheby_coeffs, cheby_step  # noqa: F401  (the entry points that launch these kernels)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spmv-cache-trace_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

SRC = '#include "cheby_updates.hpp"\n' \
      "#define STEP(T, M, K) template __global__ void spmv::cheby_step_kernel<T, M, K>(long long, const double *, const T *, const T *, T *, T *, " \
      "const T *, spmv::v2d *)\n" \
      + "".join("STEP(%s, %s, %d);\n" % (t, m, k) for t in ("double", "float") for m in ("false", "true") for k in range(6)) \
      + "".join("template __global__ void spmv::cheby_bound_kernel<%s, %s>(int, const int *, const double *, const %s *, unsigned long long *);\n"
                % (t, m, t) for t in ("double", "float") for m in ("false", "true"))
MODES = ("first", "middle", "last", "last + dots", "sole", "sole + dots")
# (type, minv): (VGPRs, waves per SIMD) of the six modes
SHIPPED = {
    ("d", 0): [(24, 8), (36, 8), (32, 8), (46, 8), (24, 8), (46, 8)],
    ("d", 1): [(40, 8), (42, 8), (42, 8), (52, 8), (38, 8), (38, 8)],
    ("f", 0): [(46, 8), (56, 8), (54, 8), (46, 8), (44, 8), (64, 8)],
    ("f", 1): [(42, 8), (44, 8), (42, 8), (54, 8), (42, 8), (58, 8)],
}


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("cheby_resources")
    src = d / "cheby.hip"
    src.write_text(SRC)
    # the Makefile's flags
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", str(src), "-o", str(d / "cheby.s")],
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


def _report(what, remark):
    print("%s: %d VGPRs, %d SGPRs, %d bytes of LDS, %d bytes of scratch, occupancy %d" % (
        what, remark(" VGPRs"), remark("TotalSGPRs"), remark("LDS Size [bytes/block]"), remark("ScratchSize [bytes/lane]"),
        remark("Occupancy [waves/SIMD]")))


def test_twenty_four_step_kernels():
    assert len(SHIPPED) == 4 and all(len(v) == len(MODES) == 6 for v in SHIPPED.values())


@pytest.mark.parametrize("t,m", sorted(SHIPPED))
def test_no_scratch_no_lds_and_the_shipped_registers_in_the_step(remarks, t, m):
    for mode, (vgprs, waves) in enumerate(SHIPPED[(t, m)]):
        remark = _remarks_of(remarks, "cheby_step_kernelI%sLb%dELi%dE" % (t, m, mode))
        _report("%s, minv %d, %s" % (t, m, MODES[mode]), remark)
        assert remark("ScratchSize [bytes/lane]") == 0
        assert remark("LDS Size [bytes/block]") == 0
        assert remark(" VGPRs") == vgprs
        assert remark("Occupancy [waves/SIMD]") == waves


def test_the_bound_and_the_coefficients_are_reported(remarks):
    for t in ("d", "f"):
        for m in (0, 1):
            _report("bound, %s, minv %d" % (t, m), _remarks_of(remarks, "cheby_bound_kernelI%sLb%dE" % (t, m)))
    _report("coefficients", _remarks_of(remarks, "cheby_coeffs_kernel"))
    _report("zeroing", _remarks_of(remarks, "cheby_zero_kernel"))
