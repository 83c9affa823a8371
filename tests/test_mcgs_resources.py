"""The kernels of the multicolour Gauss-Seidel / SSOR preconditioner (mcgs_kernels.hpp) keep their budget, read from the
compiler's resource remarks for gfx950 with the Makefile's flags alone: every instantiation of the sweep (two types x seven group
sizes) and of the dots pass is present, none uses scratch or LDS, and VGPRs and occupancy are pinned at the shipped values
(groups of four lanes and more run at 8 waves per SIMD with four passes in flight; groups of one and two lanes load
every pass's row in every lane and pay 77 registers and 6 waves for it in doubles).  The colouring, the counting sort and the
copy are one-time code: no scratch, otherwise reported, not gated.  Needs hipcc, not a GPU."""
import os
import re
import shutil
import subprocess

import pytest

from spmv_amd.capi import mcgs_apply, mcgs_sweep  # noqa: F401  (the entry points that launch these kernels)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spmv-cache-trace_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
GROUPS = (1, 2, 4, 8, 16, 32, 64)

SRC = '#include "mcgs_kernels.hpp"\n' \
      + "".join("template __global__ void spmv::mcgs_sweep_kernel<%s, %d>(int, int, const int *, const int *, const int *, const double *, double, "
                "double, const %s *, const %s *, %s *);\n" % (t, g, t, t, t) for t in ("double", "float") for g in GROUPS) \
      + "".join("template __global__ void spmv::mcgs_dots_kernel<%s>(long long, const %s *, const %s *, spmv::v2d *);\n" % (t, t, t)
                for t in ("double", "float")) \
      + "template __global__ void spmv::rounds_mark_kernel<true>(int, unsigned, const int *, const int *, const double *, const double *, const int *, " \
        "unsigned char *, int *);\n"
# type: (VGPRs, waves per SIMD) of the seven group sizes
SHIPPED = {
    "d": [(76, 6), (77, 6), (51, 8), (52, 8), (51, 8), (51, 8), (50, 8)],
    "f": [(63, 8), (65, 7), (48, 8), (49, 8), (48, 8), (48, 8), (47, 8)],
}
DOTS = {"d": (40, 8), "f": (64, 8)}
# (the marks of a colouring round are graph_rounds.hpp's rounds_mark_kernel<true>, instantiated above)
ONE_TIME = ("mcgs_init", "rounds_mark", "mcgs_assign", "mcgs_check", "mcgs_hist", "mcgs_offsets", "mcgs_scatter", "mcgs_chunk_sum", "mcgs_chunk_scan",
            "mcgs_row_scan", "mcgs_copy")


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("mcgs_resources")
    src = d / "mcgs.hip"
    src.write_text(SRC)
    # the Makefile's flags
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", str(src), "-o", str(d / "mcgs.s")],
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


@pytest.mark.parametrize("t", sorted(SHIPPED))
def test_no_scratch_no_lds_and_the_shipped_registers_in_the_sweep(remarks, t):
    assert len(SHIPPED[t]) == len(GROUPS) == 7
    for g, (vgprs, waves) in zip(GROUPS, SHIPPED[t]):
        remark = _remarks_of(remarks, "mcgs_sweep_kernelI%sLi%dEE" % (t, g))
        _report("sweep, %s, group %d" % (t, g), remark)
        assert remark("ScratchSize [bytes/lane]") == 0
        assert remark("LDS Size [bytes/block]") == 0
        assert remark(" VGPRs") == vgprs
        assert remark("Occupancy [waves/SIMD]") == waves
    remark = _remarks_of(remarks, "mcgs_dots_kernelI%sE" % t)
    _report("dots, %s" % t, remark)
    assert remark("ScratchSize [bytes/lane]") == 0 and remark("LDS Size [bytes/block]") == 0
    assert (remark(" VGPRs"), remark("Occupancy [waves/SIMD]")) == DOTS[t]


def test_the_one_time_kernels_use_no_scratch_and_are_reported(remarks):
    for name in ONE_TIME:
        remark = _remarks_of(remarks, "%s_kernel" % name)
        _report(name, remark)
        assert remark("ScratchSize [bytes/lane]") == 0
