"""The kernels of the aggregation multigrid level (agg_kernels.hpp) keep their budget, read from the compiler's resource remarks
for gfx950 with the Makefile's flags alone: the restriction and the prolongation in both types use no scratch and no LDS and run
at 8 waves per SIMD, with their VGPRs pinned at the shipped values (two aggregates, or two pieces of four elements, of a lane in
flight).  The aggregation, the member lists and the Galerkin product are one-time code: no scratch, otherwise reported, not gated.
Needs hipcc, not a GPU."""
import os
import re
import shutil
import subprocess

import pytest

from spmv_amd.capi import agg_prolong_add, agg_restrict  # noqa: F401  (the entry points that launch these kernels)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spmv-cache-trace_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

SRC = '#include "agg_kernels.hpp"\n' \
      + "".join("template __global__ void spmv::agg_restrict_kernel<%s>(int, int, const int *, const int *, const %s *, %s *);\n" % (t, t, t)
                + "template __global__ void spmv::agg_prolong_kernel<%s>(long long, double, const int *, const %s *, %s *);\n" % (t, t, t)
                for t in ("double", "float")) \
      + "template __global__ void spmv::rounds_mark_kernel<false>(int, unsigned, const int *, const int *, const double *, const double *, const int *, " \
        "unsigned char *, int *);\n"
# kernel: type: (VGPRs, waves per SIMD)
SHIPPED = {"restrict": {"d": (37, 8), "f": (37, 8)}, "prolong": {"d": (40, 8), "f": (40, 8)}}
# (the marks of a distance-1 round are graph_rounds.hpp's rounds_mark_kernel<false>, instantiated above)
ONE_TIME = ("agg_init", "rounds_mark", "agg_assign", "agg_flag", "agg_join", "agg_status", "agg_count", "agg_key", "agg_head", "agg_pattern",
            "agg_numeric")


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("agg_resources")
    src = d / "agg.hip"
    src.write_text(SRC)
    # the Makefile's flags
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", str(src), "-o", str(d / "agg.s")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    return r.stdout, (d / "agg.s").read_text()


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


@pytest.mark.parametrize("t", ["d", "f"])
@pytest.mark.parametrize("kernel", sorted(SHIPPED))
def test_no_scratch_no_lds_eight_waves_and_the_shipped_registers_in_restrict_and_prolong(remarks, kernel, t):
    remark = _remarks_of(remarks[0], "agg_%s_kernelI%sE" % (kernel, t))
    _report("%s, %s" % (kernel, t), remark)
    assert remark("ScratchSize [bytes/lane]") == 0
    assert remark("LDS Size [bytes/block]") == 0
    assert remark("Occupancy [waves/SIMD]") == 8
    assert (remark(" VGPRs"), remark("Occupancy [waves/SIMD]")) == SHIPPED[kernel][t]


def test_the_hot_kernels_load_their_indices_and_vectors_sixteen_bytes_wide(remarks):
    """agg, member and x as 16-byte loads and the member-pointer pairs as 8-byte loads: counted in each kernel's assembly."""
    for kernel, t, wide, pair in (("prolong", "d", 6, 0), ("prolong", "f", 4, 0), ("restrict", "d", 2, 1), ("restrict", "f", 2, 1)):
        m = re.search(r"^(_ZN4spmv\d+agg_%s_kernelI%sE\w*):[^\n]*\n(.*?)\n\.Lfunc_end" % (kernel, t), remarks[1], re.S | re.M)
        assert m, (kernel, t)
        body = m.group(2)
        n16, n8 = len(re.findall(r"global_load_dwordx4", body)), len(re.findall(r"global_load_dwordx2", body))
        print("%s, %s: %d 16-byte and %d 8-byte loads" % (kernel, t, n16, n8))
        assert n16 >= wide and n8 >= pair, (kernel, t, n16, n8)


def test_the_one_time_kernels_use_no_scratch_and_are_reported(remarks):
    for name in ONE_TIME:
        remark = _remarks_of(remarks[0], "%s_kernel" % name)
        _report(name, remark)
        assert remark("ScratchSize [bytes/lane]") == 0
