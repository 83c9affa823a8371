"""The kernels of include/spmv_hip_agg_mis2.h (agg_kernels.hpp) keep their budget, read from the compiler's resource remarks for
gfx950 with the Makefile's flags alone: the restriction by a group of lanes in both types and every group it is instantiated for
(2 ... 64; a group of one lane is agg_restrict_kernel, which test_agg_resources.py holds) uses no scratch and no LDS and runs at 8
waves per SIMD, with its VGPRs pinned at the shipped values (four passes of two members of a lane in flight); it loads the
member-pointer pairs 8 bytes wide.  The kernels of the distance-2 aggregation are one-time code: no scratch, otherwise reported,
not gated.  Needs hipcc, not a GPU."""
import os
import re
import shutil
import subprocess

import pytest

from spmv_amd.capi import agg_aggregate_mis2, agg_restrict_group  # noqa: F401  (the entry points that launch these kernels)
from test_agg_resources import _remarks_of, _report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spmv-cache-trace_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

GROUPS = (2, 4, 8, 16, 32, 64)
SRC = '#include "agg_kernels.hpp"\n' \
      + "".join("template __global__ void spmv::agg_restrict_group_kernel<%s, %d>(int, const int *, const int *, const %s *, %s *);\n" % (t, g, t, t)
                for t in ("double", "float") for g in GROUPS)
# type: group: VGPRs (all at 8 waves per SIMD)
SHIPPED = {"d": {2: 43, 4: 43, 8: 43, 16: 43, 32: 43, 64: 33}, "f": {2: 43, 4: 43, 8: 43, 16: 43, 32: 43, 64: 33}}
ONE_TIME = ("near", "mark", "beside", "assign", "join1", "join2")


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("agg_mis2_resources")
    src = d / "agg_mis2.hip"
    src.write_text(SRC)
    # the Makefile's flags
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", str(src), "-o", str(d / "agg_mis2.s")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    return r.stdout, (d / "agg_mis2.s").read_text()


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("t", ["d", "f"])
def test_no_scratch_no_lds_eight_waves_and_the_shipped_registers_in_the_grouped_restriction(remarks, t, group):
    remark = _remarks_of(remarks[0], "agg_restrict_group_kernelI%sLi%dEE" % (t, group))
    _report("restrict by groups of %d, %s" % (group, t), remark)
    assert remark("ScratchSize [bytes/lane]") == 0
    assert remark("LDS Size [bytes/block]") == 0
    assert remark("Occupancy [waves/SIMD]") == 8
    assert remark(" VGPRs") == SHIPPED[t][group]


def test_the_grouped_restriction_loads_the_member_pointer_pairs_eight_bytes_wide(remarks):
    """A lane's own members lie `group` words apart, so they and their gathers are single loads that the lanes of a group coalesce;
    the pair member_ptr[I], member_ptr[I + 1] is one 8-byte load per pass in flight (a double's gather is 8 bytes wide too): counted
    in each kernel's assembly.  With 64 lanes an aggregate the pair is the same for the whole wave and the compiler reads it through
    the scalar unit: reported there, not counted."""
    for t in ("d", "f"):
        for group in GROUPS:
            m = re.search(r"^(_ZN4spmv\d+agg_restrict_group_kernelI%sLi%dEE\w*):[^\n]*\n(.*?)\n\.Lfunc_end" % (t, group), remarks[1], re.S | re.M)
            assert m, (t, group)
            n8, n4 = len(re.findall(r"global_load_dwordx2", m.group(2))), len(re.findall(r"global_load_dword\b", m.group(2)))
            print("groups of %d, %s: %d 8-byte and %d 4-byte loads" % (group, t, n8, n4))
            if group < 64:
                assert n8 >= (4 if t == "f" else 4 + 8), (t, group, n8)


def test_the_one_time_kernels_use_no_scratch_and_are_reported(remarks):
    for name in ONE_TIME:
        remark = _remarks_of(remarks[0], "agg_mis2_%s_kernel" % name)
        _report(name, remark)
        assert remark("ScratchSize [bytes/lane]") == 0
